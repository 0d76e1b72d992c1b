"""Host-side mirror of the reference's interface for the association-scan path, over the C ABI.

Names follow the reference's classes (src/kmers_multiple_databases.h, src/best_associations_heap.h):

  KmersTable            <- MultipleKmersDataBases' ctor guards + .names            (a-1, a-2)
  Phenotypes            <- load_phenotypes_file                                    (a-10)
  AssociationScan       <- load_kmers + add_kmers_to_heap over all columns (pass 1) (a-3 .. a-8)
  BestAssociationsHeap  <- BestAssociationsHeap                                    (a-7)
  Kinship               <- update_emma_kinshhip_calculation / emma_kinship_kmers    (a-9)
  SnpKinship            <- emma_kinship (the kinship of a PLINK SNP matrix)          (f-5)
  filter_kmers          <- filter_kmers (rows of listed k-mers)                       (f-6)
  build_kmers_table     <- build_kmers_table (the table from sorted k-mer files)      (f-7)
  kmers_ld              -- this project's own: exact r^2 links between k-mers (clump_kmers)
  kmers_ld_proxies      -- this project's own: the rows in LD with a few lead rows, as records (proxy_kmers)
  locate_kmers_bases    -- this project's own: where in a base stream k-mers occur, exactly or with one mismatch (locate_kmers)
  fetch_reads_bases     -- this project's own: the reads of a newline-separated stream that contain listed k-mers (fetch_reads)
  fetch_reads           -- the tool's run: reads files in, the kept reads, their table and the log out

Everything numeric happens inside libkgwas (HIP kernels on the GPU + the std::priority_queue
replay); this module only moves buffers.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Sequence

import numpy as np

from . import capi
from .capi import lib, check, ptr


def min_count(n_acc: int, maf: float, mac: int) -> int:
    return int(lib.kgwas_min_count(n_acc, maf, mac))


class KmersTable:
    def __init__(self, base: str, kmer_len: int = 0):
        self._h = C.c_void_p()
        check(lib.kgwas_table_open(base.encode(), kmer_len, C.byref(self._h)))
        a, r, w, k = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint32()
        check(lib.kgwas_table_info(self._h, C.byref(a), C.byref(r), C.byref(w), C.byref(k)))
        self.base = base
        self.n_acc, self.n_rows, self.words_per_row, self.kmer_len = a.value, r.value, w.value, k.value
        self.names = []
        for i in range(self.n_acc):
            s = C.c_char_p()
            check(lib.kgwas_table_name(self._h, i, C.byref(s)))
            self.names.append(s.value.decode())

    def column_map(self, accessions: Sequence[str]) -> np.ndarray:
        arr = (C.c_char_p * len(accessions))(*[a.encode() for a in accessions])
        out = np.zeros(len(accessions), dtype=np.uint64)
        check(lib.kgwas_table_column_map(self._h, arr, len(accessions), out.ctypes.data_as(C.POINTER(C.c_uint64))))
        return out

    def read_rows(self, row0: int, n: int) -> np.ndarray:
        out = np.empty((n, 1 + self.words_per_row), dtype=np.uint64)
        check(lib.kgwas_table_read_rows(self._h, row0, n, ptr(out)))
        return out

    def close(self):
        if self._h:
            lib.kgwas_table_close(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        self.close()


class Phenotypes:
    def __init__(self, path: str):
        h = C.c_void_p()
        check(lib.kgwas_pheno_load(path.encode(), C.byref(h)))
        try:
            p, a = C.c_uint64(), C.c_uint64()
            check(lib.kgwas_pheno_info(h, C.byref(p), C.byref(a)))
            self.names, self.accessions = [], []
            s = C.c_char_p()
            for j in range(p.value):
                check(lib.kgwas_pheno_name(h, j, C.byref(s)))
                self.names.append(s.value.decode())
            for i in range(a.value):
                check(lib.kgwas_pheno_accession(h, i, C.byref(s)))
                self.accessions.append(s.value.decode())
            y = C.POINTER(C.c_float)()
            check(lib.kgwas_pheno_values(h, C.byref(y)))
            n = p.value * a.value
            self.Y = (np.ctypeslib.as_array(y, shape=(n,)).copy() if n else np.zeros(0, np.float32)).reshape(
                p.value, a.value)
        finally:
            lib.kgwas_pheno_free(h)


class BestAssociationsHeap:
    def __init__(self, max_results: int, _handle=None):
        self._h = C.c_void_p(_handle) if _handle else C.c_void_p()
        if not _handle:
            check(lib.kgwas_heap_new(max_results, C.byref(self._h)))

    def add_associations(self, kmer, score, row):
        k = np.ascontiguousarray(kmer, np.uint64)
        s = np.ascontiguousarray(score, np.float64)
        r = np.ascontiguousarray(row, np.uint64)
        check(lib.kgwas_heap_add_many(self._h, ptr(k), ptr(s), ptr(r), len(k)))

    def add_association(self, kmer, score, row):
        self.add_associations([kmer], [score], [row])

    def _size(self):
        n, ins, low = C.c_uint64(), C.c_uint64(), C.c_double()
        check(lib.kgwas_heap_size(self._h, C.byref(n), C.byref(ins), C.byref(low)))
        return n.value, ins.value, low.value

    def __len__(self):
        return self._size()[0]

    @property
    def lowest_score(self):
        return self._size()[2]

    def pop_all(self):
        n = len(self)
        k, s, r = np.zeros(n, np.uint64), np.zeros(n, np.float64), np.zeros(n, np.uint64)
        check(lib.kgwas_heap_pop_all(self._h, ptr(k), ptr(s), ptr(r)))
        return k, s, r

    def get_kmers_for_output(self):
        n = len(self)
        k, rk, r = np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.zeros(n, np.uint64)
        check(lib.kgwas_heap_output_list(self._h, ptr(k), ptr(rk), ptr(r)))
        return k, rk, r

    def get_rows_sorted_indices(self):
        """src/best_associations_heap.cpp:135-147."""
        r = np.zeros(len(self), np.uint64)
        check(lib.kgwas_heap_rows_sorted(self._h, ptr(r)))
        return r

    def output_to_file(self, path: str, with_scores: bool = False):
        """output_to_file / output_to_file_with_scores (src/best_associations_heap.cpp:65-90)."""
        check(lib.kgwas_heap_output_to_file(self._h, path.encode(), 1 if with_scores else 0))

    def __del__(self):
        if getattr(self, "_h", None):
            lib.kgwas_heap_free(self._h)
            self._h = None


class AssociationScan:
    """Pass 1 of associate_kmers for all phenotype columns at once.
    record_history: what a shard other than the first keeps for a cross-shard merge (kmersgwas_amd.dist): 1 / True =
    every effective heap push (history(), history_above()); 2 = each heap's last evictions only (history_above()
    alone, 6 % of a pass instead of 14 %; raises if the ring - KGWAS_HISTORY_RING, default 4096 - was too short)."""

    def __init__(self, n_acc_file: int, col, Y, topn, min_count: int, device: int = 0, kernel: int = capi.KERNEL_AUTO,
                 chunk_rows: int = 0, host_threads: int = 0, record_history: int = 0,
                 count_patterns: bool = False):
        self.col = np.ascontiguousarray(col, np.uint64)
        self.Y = np.ascontiguousarray(Y, np.float32)
        if self.Y.ndim == 1:
            self.Y = self.Y[None, :]
        self.n_pheno, self.n_acc = self.Y.shape
        self.topn = np.ascontiguousarray(np.broadcast_to(np.asarray(topn, np.uint64), (self.n_pheno,)))
        self.n_acc_file = n_acc_file
        self.words_per_row = (n_acc_file + 63) // 64
        p = capi.ScanParams()
        p.struct_size = C.sizeof(capi.ScanParams)
        p.device = device
        p.n_acc_file = n_acc_file
        p.n_acc = self.n_acc
        p.col = self.col.ctypes.data_as(C.POINTER(C.c_uint64))
        p.n_pheno = self.n_pheno
        p.Y = self.Y.ctypes.data_as(C.POINTER(C.c_float))
        p.topn = self.topn.ctypes.data_as(C.POINTER(C.c_uint64))
        p.min_count = min_count
        p.chunk_rows = chunk_rows
        p.host_threads = host_threads
        p.kernel = kernel
        p.record_history = int(record_history)  # False/0 off, True/1 full log, 2 eviction ring
        p.count_patterns = 1 if count_patterns else 0
        self._h = C.c_void_p()
        check(lib.kgwas_scan_create(C.byref(p), C.byref(self._h)))
        # columns may be finished by selection instead of the push-by-push replay (kmersgwas_amd/csrc/scan_lazy.cpp): what
        # kmersgwas_amd.dist.merge_shards looks at (it must come out the same on every rank of a merge). Asked of the library:
        # sessions that fell back to the exact scorers (non-finite phenotypes, an explicit kernel) are NOT in select mode.
        on = C.c_int(0)
        check(lib.kgwas_scan_select_mode(self._h, C.byref(on)))
        self.select_mode = bool(on.value)

    # rows: uint64 array (n_rows, 1 + W_f) in host memory
    def feed_host(self, rows: np.ndarray, first_row: int = 0):
        rows = np.ascontiguousarray(rows, np.uint64)
        n = rows.size // (1 + self.words_per_row)
        check(lib.kgwas_scan_feed_host(self._h, ptr(rows), n, first_row))

    def feed_table(self, table: "KmersTable", row0: int, n_rows: int):
        """Rows [row0, row0 + n_rows) of an open table, read / copied / scored in overlapping 128 MiB pieces."""
        check(lib.kgwas_scan_feed_table(self._h, table._h, row0, n_rows))

    # device pointer to rows already resident in HBM (e.g. torch tensor .data_ptr())
    def expect_finish(self):
        """Hint: the next feed is the last one before finish(); the replay workers that run out of records near its end
        then pop complete columns into the result lists while the slowest worker is still replaying (results unchanged)."""
        check(lib.kgwas_scan_expect_finish(self._h))

    def feed_device(self, d_ptr: int, n_rows: int, first_row: int = 0, stream: int = 0):
        check(lib.kgwas_scan_feed_device(self._h, C.c_void_p(d_ptr), n_rows, first_row, C.c_void_p(stream)))

    def finish(self):
        check(lib.kgwas_scan_finish(self._h))

    def reset(self):
        """Empty heaps / histories / statistics, keep all buffers (session reuse)."""
        check(lib.kgwas_scan_reset(self._h))

    def lowest(self):
        """(lowest_score[n_pheno], full[n_pheno]) of the heaps as they stand."""
        low = np.zeros(self.n_pheno, np.float64)
        full = np.zeros(self.n_pheno, np.uint8)
        check(lib.kgwas_scan_lowest(self._h, ptr(low), ptr(full)))
        return low, full.astype(bool)

    def absorb(self, shard_histories):
        """Replay later shards' (pre-filtered) histories, in shard order, into this scan's heaps.
        shard_histories[g][j] = (kmer, score, row). Call finish() again afterwards."""
        G = len(shard_histories)
        if G == 0:
            return
        P = self.n_pheno
        counts = np.zeros((G, P), np.uint64)
        ks, ss, rs = [], [], []
        for g in range(G):
            for j in range(P):
                counts[g, j] = len(shard_histories[g][j][0])
            ks.append(np.ascontiguousarray(np.concatenate([np.asarray(h[0], np.uint64) for h in shard_histories[g]])))
            ss.append(np.ascontiguousarray(np.concatenate([np.asarray(h[1], np.float64) for h in shard_histories[g]])))
            rs.append(np.ascontiguousarray(np.concatenate([np.asarray(h[2], np.uint64) for h in shard_histories[g]])))
        kp = (C.c_void_p * G)(*[a.ctypes.data for a in ks])
        sp = (C.c_void_p * G)(*[a.ctypes.data for a in ss])
        rp = (C.c_void_p * G)(*[a.ctypes.data for a in rs])
        check(lib.kgwas_scan_absorb(self._h, G, ptr(counts), kp, sp, rp))

    def absorb_flat(self, counts: np.ndarray, kmer: Sequence[np.ndarray], score: Sequence[np.ndarray], row: Sequence[np.ndarray]):
        """absorb() on flat arrays: counts[g][j] entries of column j in shard g, shard g's entries concatenated by
        column in kmer[g] / score[g] / row[g]."""
        counts = np.ascontiguousarray(counts, np.uint64)
        G = counts.shape[0]
        if G == 0:
            return
        ks = [np.ascontiguousarray(a, np.uint64) for a in kmer]
        ss = [np.ascontiguousarray(a, np.float64) for a in score]
        rs = [np.ascontiguousarray(a, np.uint64) for a in row]
        kp = (C.c_void_p * G)(*[a.ctypes.data for a in ks])
        sp = (C.c_void_p * G)(*[a.ctypes.data for a in ss])
        rp = (C.c_void_p * G)(*[a.ctypes.data for a in rs])
        check(lib.kgwas_scan_absorb(self._h, G, ptr(counts), kp, sp, rp))

    def _flat3(self, total, k, s, r):
        """Views of the library's export scratch: valid until the next history_above / heaps_export call."""
        if total == 0:
            return np.zeros(0, np.uint64), np.zeros(0, np.float64), np.zeros(0, np.uint64)
        return (np.ctypeslib.as_array(k, (total,)), np.ctypeslib.as_array(s, (total,)), np.ctypeslib.as_array(r, (total,)))

    def history_above(self, thr: np.ndarray):
        """Recorded history entries with score > thr[j] (thr = -inf keeps all), flat by column:
        (counts[P], kmer, score, row)."""
        thr = np.ascontiguousarray(thr, np.float64)
        counts = np.zeros(self.n_pheno, np.uint64)
        k, s, r = C.POINTER(C.c_uint64)(), C.POINTER(C.c_double)(), C.POINTER(C.c_uint64)()
        check(lib.kgwas_scan_history_above(self._h, ptr(thr), ptr(counts), C.byref(k), C.byref(s), C.byref(r)))
        return (counts,) + self._flat3(int(counts.sum()), k, s, r)

    def heaps_export(self, cols):
        """State of the heaps `cols` in heap-array order, flat: (sizes[len(cols)], kmer, score, row)."""
        cols = np.ascontiguousarray(cols, np.uint64)
        sizes = np.zeros(len(cols), np.uint64)
        k, s, r = C.POINTER(C.c_uint64)(), C.POINTER(C.c_double)(), C.POINTER(C.c_uint64)()
        check(lib.kgwas_scan_heaps_export(self._h, len(cols), ptr(cols), ptr(sizes), C.byref(k), C.byref(s), C.byref(r)))
        return (sizes,) + self._flat3(int(sizes.sum()), k, s, r)

    @staticmethod
    def _msg_args(col0, ncols, out):
        col0 = np.ascontiguousarray(col0, np.uint64)
        ncols = np.ascontiguousarray(ncols, np.uint64)
        assert len(col0) == len(ncols)
        words = np.zeros(len(col0), np.uint64)
        if out is None:
            return col0, ncols, words, None, 0
        assert out.dtype.itemsize == 8 and out.ndim == 1 and out.flags["C_CONTIGUOUS"] and out.flags["WRITEABLE"]
        return col0, ncols, words, C.c_void_p(out.ctypes.data), len(out)

    def history_above_msgs(self, thr: np.ndarray, col0, ncols, out):
        """history_above() as messages written into `out` (a 1-D array of 64-bit words, e.g. a view of a pinned staging
        buffer; include/kgwas.h describes the layout): message m = the columns col0[m] .. col0[m] + ncols[m] - 1.
        Returns the messages' lengths in words; nothing was written if their sum exceeds len(out)."""
        thr = np.ascontiguousarray(thr, np.float64)
        assert len(thr) == self.n_pheno
        col0, ncols, words, p_out, cap = self._msg_args(col0, ncols, out)
        check(lib.kgwas_scan_history_above_msgs(self._h, ptr(thr), len(col0), ptr(col0), ptr(ncols), p_out, cap, ptr(words)))
        return words

    def heaps_export_msgs(self, col0, ncols, out):
        """heaps_export() as messages written into `out` (see history_above_msgs)."""
        col0, ncols, words, p_out, cap = self._msg_args(col0, ncols, out)
        check(lib.kgwas_scan_heaps_export_msgs(self._h, len(col0), ptr(col0), ptr(ncols), p_out, cap, ptr(words)))
        return words

    def heaps_import(self, cols, sizes, kmer, score, row):
        """Re-create exported heap states (layout included) in this session. Call finish() again afterwards."""
        cols = np.ascontiguousarray(cols, np.uint64)
        sizes = np.ascontiguousarray(sizes, np.uint64)
        kmer = np.ascontiguousarray(kmer, np.uint64)
        score = np.ascontiguousarray(score, np.float64)
        row = np.ascontiguousarray(row, np.uint64)
        assert len(kmer) == len(score) == len(row) == int(sizes.sum())
        check(lib.kgwas_scan_heaps_import(self._h, len(cols), ptr(cols), ptr(sizes), ptr(kmer), ptr(score), ptr(row)))

    def _lists(self, fn, j):
        n = C.c_uint64()
        k, s, r = C.POINTER(C.c_uint64)(), C.POINTER(C.c_double)(), C.POINTER(C.c_uint64)()
        check(fn(self._h, j, C.byref(n), C.byref(k), C.byref(s), C.byref(r)))
        m = n.value
        if m == 0:
            return np.zeros(0, np.uint64), np.zeros(0, np.float64), np.zeros(0, np.uint64)
        return (np.ctypeslib.as_array(k, shape=(m,)).copy(), np.ctypeslib.as_array(s, shape=(m,)).copy(),
                np.ctypeslib.as_array(r, shape=(m,)).copy())

    def result(self, j: int):
        """(kmers, scores, file rows) of column j in heap-pop order (ascending score; rank of entry i = n - i)."""
        return self._lists(lib.kgwas_scan_result, j)

    def history(self, j: int):
        return self._lists(lib.kgwas_scan_history, j)

    def stats(self) -> dict:
        st = capi.ScanStats()
        check(lib.kgwas_scan_get_stats(self._h, C.byref(st)))
        return st.as_dict()

    def scores_dense(self, rows=None, d_ptr: int = 0, n_rows: int = 0):
        """calculate_kmer_score for every row x column. Returns (scores[n_pheno, n_rows], popcnt[n_rows])."""
        if rows is not None:
            rows = np.ascontiguousarray(rows, np.uint64)
            n_rows = rows.size // (1 + self.words_per_row)
            src, on_dev = ptr(rows), 0
        else:
            src, on_dev = C.c_void_p(d_ptr), 1
        sc = np.zeros((self.n_pheno, n_rows), np.float64)
        pc = np.zeros(n_rows, np.uint32)
        check(lib.kgwas_scan_scores_dense(self._h, src, on_dev, n_rows, ptr(sc), ptr(pc)))
        return sc, pc

    def close(self):
        if getattr(self, "_h", None):
            lib.kgwas_scan_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()


class MultiDeviceScan:
    """kgwas_multiscan: pass 1 of associate_kmers with the table row-sharded over `devices` (one entry per shard; a
    device may appear more than once) inside this process - what `associate_kmers --gpus N` runs."""

    def __init__(self, n_acc_file: int, col, Y, topn, min_count: int, devices: Sequence[int], kernel: int = capi.KERNEL_AUTO,
                 chunk_rows: int = 0, host_threads: int = 0, count_patterns: bool = False):
        self.col = np.ascontiguousarray(col, np.uint64)
        self.Y = np.ascontiguousarray(Y, np.float32)
        if self.Y.ndim == 1:
            self.Y = self.Y[None, :]
        self.n_pheno, self.n_acc = self.Y.shape
        self.topn = np.ascontiguousarray(np.broadcast_to(np.asarray(topn, np.uint64), (self.n_pheno,)))
        self.devices = np.ascontiguousarray(devices, np.int32)
        self.words_per_row = (n_acc_file + 63) // 64
        p = capi.ScanParams()
        p.struct_size = C.sizeof(capi.ScanParams)
        p.device = 0
        p.n_acc_file = n_acc_file
        p.n_acc = self.n_acc
        p.col = self.col.ctypes.data_as(C.POINTER(C.c_uint64))
        p.n_pheno = self.n_pheno
        p.Y = self.Y.ctypes.data_as(C.POINTER(C.c_float))
        p.topn = self.topn.ctypes.data_as(C.POINTER(C.c_uint64))
        p.min_count = min_count
        p.chunk_rows = chunk_rows
        p.host_threads = host_threads
        p.kernel = kernel
        p.record_history = 0
        p.count_patterns = 1 if count_patterns else 0
        self._h = C.c_void_p()
        check(lib.kgwas_multiscan_create(C.byref(p), ptr(self.devices), len(self.devices), C.byref(self._h)))

    def run_table(self, table: "KmersTable", row0: int, n_rows: int):
        check(lib.kgwas_multiscan_run_table(self._h, table._h, row0, n_rows))

    def run_device(self, d_ptrs: Sequence[int], n_rows: Sequence[int], first_rows: Sequence[int]):
        G = len(self.devices)
        pp = (C.c_void_p * G)(*[C.c_void_p(int(x)) for x in d_ptrs])
        nr = np.ascontiguousarray(n_rows, np.uint64)
        fr = np.ascontiguousarray(first_rows, np.uint64)
        check(lib.kgwas_multiscan_run_device(self._h, pp, ptr(nr), ptr(fr)))

    def finish(self):
        check(lib.kgwas_multiscan_finish(self._h))

    def result(self, j: int):
        n = C.c_uint64()
        k, s, r = C.POINTER(C.c_uint64)(), C.POINTER(C.c_double)(), C.POINTER(C.c_uint64)()
        check(lib.kgwas_multiscan_result(self._h, j, C.byref(n), C.byref(k), C.byref(s), C.byref(r)))
        m = n.value
        if m == 0:
            return np.zeros(0, np.uint64), np.zeros(0, np.float64), np.zeros(0, np.uint64)
        return (np.ctypeslib.as_array(k, shape=(m,)).copy(), np.ctypeslib.as_array(s, shape=(m,)).copy(),
                np.ctypeslib.as_array(r, shape=(m,)).copy())

    def stats(self) -> dict:
        G = len(self.devices)
        tot = capi.ScanStats()
        per = (capi.ScanStats * G)()
        sm, mm, rs = C.c_double(), C.c_double(), C.c_uint64()
        check(lib.kgwas_multiscan_get_stats(self._h, C.byref(tot), per, C.byref(sm), C.byref(mm), C.byref(rs)))
        d = tot.as_dict()
        d.update(scan_ms=sm.value, merge_ms=mm.value, rescans=rs.value, per_shard=[x.as_dict() for x in per])
        return d

    def close(self):
        if getattr(self, "_h", None):
            lib.kgwas_multiscan_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()


def kinship_table_multi(table: "KmersTable", min_count: int, devices: Sequence[int]):
    """emma_kinship_kmers' accumulation over the whole table, row-sharded over `devices`: (K, n_used)."""
    dv = np.ascontiguousarray(devices, np.int32)
    H = np.zeros((table.n_acc, table.n_acc), np.uint64)
    n = C.c_uint64()
    check(lib.kgwas_kinship_table_multi(ptr(dv), len(dv), table._h, min_count, ptr(H), C.byref(n)))
    return kinship_from_partials(H, n.value), n.value


def merge_shards(topn, shard_histories, threads: int = 0):
    """Cross-shard merge. shard_histories[g][j] = (kmer, score, row) arrays of shard g (row order),
    shards listed in row order. Returns one BestAssociationsHeap per phenotype column."""
    G = len(shard_histories)
    P = len(shard_histories[0])
    topn = np.ascontiguousarray(np.broadcast_to(np.asarray(topn, np.uint64), (P,)))
    counts = np.zeros((G, P), np.uint64)
    ks, ss, rs = [], [], []
    for g in range(G):
        for j in range(P):
            counts[g, j] = len(shard_histories[g][j][0])
        ks.append(np.ascontiguousarray(np.concatenate([np.asarray(h[0], np.uint64) for h in shard_histories[g]])))
        ss.append(np.ascontiguousarray(np.concatenate([np.asarray(h[1], np.float64) for h in shard_histories[g]])))
        rs.append(np.ascontiguousarray(np.concatenate([np.asarray(h[2], np.uint64) for h in shard_histories[g]])))
    kp = (C.c_void_p * G)(*[a.ctypes.data for a in ks])
    sp = (C.c_void_p * G)(*[a.ctypes.data for a in ss])
    rp = (C.c_void_p * G)(*[a.ctypes.data for a in rs])
    out = (C.c_void_p * P)()
    check(lib.kgwas_merge_shards(P, ptr(topn), G, ptr(counts), kp, sp, rp, threads, out))
    return [BestAssociationsHeap(0, _handle=out[j]) for j in range(P)]


class Kinship:
    def __init__(self, n_acc_file: int, min_count: int, device: int = 0):
        self.n_acc = n_acc_file
        self.words_per_row = (n_acc_file + 63) // 64
        self._h = C.c_void_p()
        check(lib.kgwas_kinship_create(device, n_acc_file, min_count, C.byref(self._h)))

    def feed_host(self, rows: np.ndarray):
        rows = np.ascontiguousarray(rows, np.uint64)
        check(lib.kgwas_kinship_feed_host(self._h, ptr(rows), rows.size // (1 + self.words_per_row)))

    def feed_table(self, table: "KmersTable", row0: int, n_rows: int):
        """Rows [row0, row0 + n_rows) of an open table; file read, copy and kernels of consecutive pieces overlap."""
        check(lib.kgwas_kinship_feed_table(self._h, table._h, row0, n_rows))

    def feed_device(self, d_ptr: int, n_rows: int, stream: int = 0):
        check(lib.kgwas_kinship_feed_device(self._h, C.c_void_p(d_ptr), n_rows, C.c_void_p(stream)))

    def partials(self):
        H = np.zeros((self.n_acc, self.n_acc), np.uint64)
        n = C.c_uint64()
        check(lib.kgwas_kinship_partials(self._h, ptr(H), C.byref(n)))
        return H, n.value

    def matrix(self):
        H, n = self.partials()
        return kinship_from_partials(H, n), n

    def stats(self):
        ms, l, r = C.c_double(), C.c_uint64(), C.c_uint64()
        check(lib.kgwas_kinship_get_stats(self._h, C.byref(ms), C.byref(l), C.byref(r)))
        return dict(kernel_ms=ms.value, launches=l.value, rows_fed=r.value)

    def close(self):
        if getattr(self, "_h", None):
            lib.kgwas_kinship_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()


class LmmLrt:
    """Mixed-model ML likelihood-ratio test (what the pipeline takes from `gemma -lmm 2`) of .bed variants on the GPU.

    K is eigendecomposed once (host threads); every phenotype and .bed given to the object reuses that."""

    def __init__(self, K: np.ndarray, device: int = 0, lmin: float = 1e-5, lmax: float = 1e5, chunk_variants: int = 10240,
                 covariates=None):
        K = np.ascontiguousarray(K, np.float64)
        if K.ndim != 2 or K.shape[0] != K.shape[1]:
            raise ValueError("K must be square")
        self.n = K.shape[0]
        self._h = C.c_void_p()
        check(lib.kgwas_lmm_create(self.n, ptr(K), device, lmin, lmax, chunk_variants, C.byref(self._h)))
        if covariates is not None:
            self.set_covariates(covariates)

    def set_covariates(self, W):
        """W: (n, q) covariates, 1 <= q <= 8, whose columns span the constant vector (give it a column of 1s): the model becomes
        y = W a + x b + u + e for null, null_reml, test, test_all and test_table. None restores the intercept alone. The
        multi-phenotype passes refuse an object with covariates."""
        if W is None:
            check(lib.kgwas_lmm_set_covariates(self._h, 0, None))
            return
        W = np.ascontiguousarray(W, np.float64)
        if W.ndim == 1:
            W = W[:, None]
        if W.ndim != 2 or W.shape[0] != self.n:
            raise ValueError("covariates must have one row per individual")
        W = np.ascontiguousarray(W)
        check(lib.kgwas_lmm_set_covariates(self._h, W.shape[1], ptr(W)))

    def _y(self, y):
        y = np.ascontiguousarray(y, np.float64)
        if y.shape != (self.n,):
            raise ValueError("y must have one value per individual")
        return y

    def null(self, y):
        """(log-likelihood, lambda) of the null model."""
        l0, lam0 = C.c_double(), C.c_double()
        check(lib.kgwas_lmm_null(self._h, ptr(self._y(y)), C.byref(l0), C.byref(lam0)))
        return l0.value, lam0.value

    def test(self, bed, y, maf: float = 0.0, miss: float = 1.0):
        """bed: the .bed body as bytes or a uint8 array of (n + 3) // 4 bytes per variant. Returns a dict of numpy arrays
        lrt, lambda, p, af, n_miss, tested (lrt, lambda and p are NaN where tested is False)."""
        bps = (self.n + 3) // 4
        body = np.frombuffer(bed, np.uint8) if isinstance(bed, (bytes, bytearray, memoryview)) else np.ascontiguousarray(bed, np.uint8)
        if body.size % bps:
            raise ValueError("the .bed body is not a whole number of variants of %d bytes" % bps)
        m = body.size // bps
        lrt, lam, p, af = (np.zeros(m) for _ in range(4))
        n_miss, tested = np.zeros(m, np.uint32), np.zeros(m, np.uint8)
        check(lib.kgwas_lmm_test_bed(self._h, ptr(self._y(y)), ptr(body), m, maf, miss, ptr(lrt), ptr(lam), ptr(p), ptr(af),
                                     ptr(n_miss), ptr(tested)))
        return {"lrt": lrt, "lambda": lam, "p": p, "af": af, "n_miss": n_miss, "tested": tested.astype(bool)}

    def null_reml(self, y):
        """The null model by REML (`-lmm 4`): (log restricted likelihood, lambda, vg, ve), ve = yy.w / (n - 1) and vg = lambda ve
        at the maximiser - emma.REMLE's vg and ve."""
        v = [C.c_double() for _ in range(4)]
        check(lib.kgwas_lmm_null_reml(self._h, ptr(self._y(y)), *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def test_all(self, bed, y, maf: float = 0.0, miss: float = 1.0):
        """test with the numbers of `-lmm 4` beside the LRT: beta (the REML effect estimate per unit of the decoded dosage), se,
        lambda_remle, p_wald (both tests at lambda_remle) and p_score (at the null model's ML lambda). lrt, lambda, p, af, n_miss and
        tested have the bits test gives; all eight statistics are NaN where tested is False."""
        bps = (self.n + 3) // 4
        body = np.frombuffer(bed, np.uint8) if isinstance(bed, (bytes, bytearray, memoryview)) else np.ascontiguousarray(bed, np.uint8)
        if body.size % bps:
            raise ValueError("the .bed body is not a whole number of variants of %d bytes" % bps)
        m = body.size // bps
        lrt, lam, p, beta, se, lam_r, p_wald, p_score, af = (np.zeros(m) for _ in range(9))
        n_miss, tested = np.zeros(m, np.uint32), np.zeros(m, np.uint8)
        check(lib.kgwas_lmm_test_bed_all(self._h, ptr(self._y(y)), ptr(body), m, maf, miss, ptr(lrt), ptr(lam), ptr(p), ptr(beta), ptr(se),
                                         ptr(lam_r), ptr(p_wald), ptr(p_score), ptr(af), ptr(n_miss), ptr(tested)))
        return {"lrt": lrt, "lambda": lam, "p": p, "beta": beta, "se": se, "lambda_remle": lam_r, "p_wald": p_wald, "p_score": p_score,
                "af": af, "n_miss": n_miss, "tested": tested.astype(bool)}

    def test_bed_multi(self, Y, bed, maf: float = 0.0, miss: float = 1.0):
        """Y: (P, n), P phenotype columns tested against one .bed body (as in test) in one pass over it. Returns a dict of
        numpy arrays: lrt, lambda, p of shape (P, M), logl0, lambda0 of shape (P,), af, n_miss, tested of shape (M,). Every value
        has the bits of null(Y[k]) / test(bed, Y[k])."""
        Y = np.ascontiguousarray(Y, np.float64)
        if Y.ndim != 2 or Y.shape[1] != self.n:
            raise ValueError("Y must have one row per phenotype column and one value per individual")
        bps = (self.n + 3) // 4
        body = np.frombuffer(bed, np.uint8) if isinstance(bed, (bytes, bytearray, memoryview)) else np.ascontiguousarray(bed, np.uint8)
        if body.size % bps:
            raise ValueError("the .bed body is not a whole number of variants of %d bytes" % bps)
        m, P = body.size // bps, Y.shape[0]
        lrt, lam, p = (np.zeros((P, m)) for _ in range(3))
        l0, lam0, af = np.zeros(P), np.zeros(P), np.zeros(m)
        n_miss, tested = np.zeros(m, np.uint32), np.zeros(m, np.uint8)
        check(lib.kgwas_lmm_test_bed_multi(self._h, P, ptr(Y), ptr(body), m, maf, miss, ptr(lrt), ptr(lam), ptr(p), ptr(l0), ptr(lam0),
                                           ptr(af), ptr(n_miss), ptr(tested)))
        return {"lrt": lrt, "lambda": lam, "p": p, "logl0": l0, "lambda0": lam0, "af": af, "n_miss": n_miss, "tested": tested.astype(bool)}

    def test_table(self, table: "KmersTable", col, y, min_count: int, maf: float = 0.0, best_n: int = 10001, max_patterns=None):
        """The exact test of every k-mer of a k-mers table (col: the table column of every individual, in order) and the best
        best_n of them by lrt, ties to the earlier row. A row is tested iff table_to_bed would write it at min_count and test
        would test its .bed row at maf; the numbers have the bits of that route. Returns a dict of numpy arrays in table row
        order: row, kmer, lrt, lambda, p, af, and the counts rows_read, rows_tested. With max_patterns (>= 64) each distinct
        presence/absence pattern is tested once and the rows that repeat it take its result from a cache of that many slots
        (rounded down to a power of two): the same dict, byte for byte, plus `unique`, a dict of the cache's counters (slots,
        patterns_cached, rows_from_cache, rows_collided, rows_rejected, rows_rotated)."""
        col = np.ascontiguousarray(col, np.uint64)
        row, kmer = np.zeros(best_n, np.uint64), np.zeros(best_n, np.uint64)
        lrt, lam, p, af = (np.zeros(best_n) for _ in range(4))
        kept, n_read, n_tested = C.c_uint64(), C.c_uint64(), C.c_uint64()
        args = (self._h, ptr(self._y(y)), table._h, ptr(col), len(col), min_count, maf, best_n, ptr(row), ptr(kmer), ptr(lrt), ptr(lam),
                ptr(p), ptr(af), C.byref(kept), C.byref(n_read), C.byref(n_tested))
        if max_patterns is None:
            check(lib.kgwas_lmm_test_table(*args))
        else:
            us = capi.LmmUniqueStats()
            check(lib.kgwas_lmm_test_table_unique(*args, int(max_patterns), C.byref(us)))
        k = kept.value
        res = {"row": row[:k], "kmer": kmer[:k], "lrt": lrt[:k], "lambda": lam[:k], "p": p[:k], "af": af[:k],
               "rows_read": n_read.value, "rows_tested": n_tested.value}
        if max_patterns is not None:
            res["unique"] = us.as_dict()
        return res

    def test_table_multi(self, table: "KmersTable", col, Y, min_count: int, maf: float = 0.0, best_n: int = 10001, max_patterns=None):
        """test_table for the P columns Y (P, n) in one pass over the table: the phenotype and its permutations. Returns a dict:
        columns, a list of P dicts shaped like test_table's (each with the rows and the bits test_table(.., Y[k], ..) gives);
        logl0 and lambda0 of shape (P,) with the bits of null(Y[k]); rows_read, rows_tested; and pairs_shipped, the number of
        (column, row) records the device's selection handed to the host (at most rows_tested * P). With max_patterns: see
        test_table_multi_skip."""
        col = np.ascontiguousarray(col, np.uint64)
        Y = np.ascontiguousarray(Y, np.float64)
        if Y.ndim != 2 or Y.shape[1] != self.n:
            raise ValueError("Y must have one row per phenotype column and one value per individual")
        P = Y.shape[0]
        row, kmer = np.zeros((P, best_n), np.uint64), np.zeros((P, best_n), np.uint64)
        lrt, lam, p, af = (np.zeros((P, best_n)) for _ in range(4))
        kept, l0, lam0 = np.zeros(P, np.uint64), np.zeros(P), np.zeros(P)
        n_read, n_tested, shipped = C.c_uint64(), C.c_uint64(), C.c_uint64()
        args = (self._h, P, ptr(Y), table._h, ptr(col), len(col), min_count, maf, best_n, ptr(row), ptr(kmer), ptr(lrt), ptr(lam), ptr(p),
                ptr(af), ptr(kept), ptr(l0), ptr(lam0), C.byref(n_read), C.byref(n_tested), C.byref(shipped))
        if max_patterns is None:
            check(lib.kgwas_lmm_test_table_multi(*args))
        else:
            ks = capi.LmmSkipStats()
            check(lib.kgwas_lmm_test_table_multi_skip(*args, int(max_patterns), C.byref(ks)))
        cols = []
        for j in range(P):
            k = int(kept[j])
            cols.append({"row": row[j, :k].copy(), "kmer": kmer[j, :k].copy(), "lrt": lrt[j, :k].copy(), "lambda": lam[j, :k].copy(),
                         "p": p[j, :k].copy(), "af": af[j, :k].copy(), "rows_read": n_read.value, "rows_tested": n_tested.value})
        res = {"columns": cols, "logl0": l0, "lambda0": lam0, "rows_read": n_read.value, "rows_tested": n_tested.value,
               "pairs_shipped": shipped.value}
        if max_patterns is not None:
            res["skip"] = ks.as_dict()
        return res

    def test_table_multi_skip(self, table: "KmersTable", col, Y, min_count: int, maf: float = 0.0, best_n: int = 10001,
                              max_patterns: int = 1 << 20):
        """test_table_multi that leaves out the rows whose presence/absence pattern is dead: an earlier row with it met full heaps
        in every column and entered none, so no later row with it can. A table of max_patterns slots (>= 64, rounded down to a
        power of two) on the device remembers the patterns. The same dict, byte for byte, plus `skip`, a dict of the table's
        counters (slots, patterns_cached, patterns_dead, rows_skipped, rows_collided, rows_rejected, rows_rotated; rows_tested =
        rows_rotated + rows_skipped)."""
        return self.test_table_multi(table, col, Y, min_count, maf, best_n, max_patterns=max_patterns)

    def stats(self):
        st = capi.LmmStats()
        check(lib.kgwas_lmm_get_stats(self._h, C.byref(st)))
        return st.as_dict()

    def close(self):
        if getattr(self, "_h", None):
            lib.kgwas_lmm_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()


def sym_eigen(K: np.ndarray, threads: int = 0):
    """K = U diag(d) U^T on host threads: (d ascending, U with eigenvectors in columns)."""
    K = np.ascontiguousarray(K, np.float64)
    n = K.shape[0]
    d, U = np.zeros(n), np.zeros((n, n))
    check(lib.kgwas_sym_eigen(n, ptr(K), ptr(d), ptr(U), threads))
    return d, U


def kinship_from_partials(H: np.ndarray, n_used: int) -> np.ndarray:
    H = np.ascontiguousarray(H, np.uint64)
    K = np.zeros_like(H)
    check(lib.kgwas_kinship_from_partials(H.shape[0], ptr(H), n_used, ptr(K)))
    return K


def kinship_format(K: np.ndarray, n_used: int) -> bytes:
    K = np.ascontiguousarray(K, np.uint64)
    need = lib.kgwas_kinship_format(K.shape[0], ptr(K), n_used, None, 0)
    buf = C.create_string_buffer(int(need) + 1)
    lib.kgwas_kinship_format(K.shape[0], ptr(K), n_used, buf, need)
    return buf.raw[:need]


def write_plink(out_base: str, table: KmersTable, col, acc_names, y, kmer_pop, row_pop):
    col = np.ascontiguousarray(col, np.uint64)
    y = np.ascontiguousarray(y, np.float32)
    kmer_pop = np.ascontiguousarray(kmer_pop, np.uint64)
    row_pop = np.ascontiguousarray(row_pop, np.uint64)
    arr = (C.c_char_p * len(acc_names))(*[a.encode() for a in acc_names])
    check(lib.kgwas_write_plink(out_base.encode(), table._h, ptr(col), len(col), arr, ptr(y), len(kmer_pop),
                                ptr(kmer_pop), ptr(row_pop)))


def write_plink_many(out_bases, table: KmersTable, col, acc_names, Y, kmer_pops, row_pops, threads: int = 0):
    """Pass 2 for all phenotype columns at once: column j's .bed/.bim/.fam from (kmer_pops[j], row_pops[j]) in pop order."""
    col = np.ascontiguousarray(col, np.uint64)
    Y = np.ascontiguousarray(Y, np.float32)
    n = len(out_bases)
    assert Y.shape == (n, len(col)) and len(kmer_pops) == n and len(row_pops) == n
    ks = [np.ascontiguousarray(k, np.uint64) for k in kmer_pops]
    rs = [np.ascontiguousarray(r, np.uint64) for r in row_pops]
    n_win = np.asarray([len(k) for k in ks], np.uint64)
    bases = (C.c_char_p * n)(*[b.encode() for b in out_bases])
    names = (C.c_char_p * len(acc_names))(*[a.encode() for a in acc_names])
    kp = (C.c_void_p * n)(*[a.ctypes.data for a in ks])
    rp = (C.c_void_p * n)(*[a.ctypes.data for a in rs])
    check(lib.kgwas_write_plink_many(n, bases, table._h, ptr(col), len(col), names, ptr(Y), ptr(n_win), kp, rp, threads))


def synth_rows_host(first_row: int, n_rows: int, n_acc: int, seed: int) -> np.ndarray:
    out = np.empty((n_rows, 1 + (n_acc + 63) // 64), np.uint64)
    check(lib.kgwas_synth_rows_host(ptr(out), first_row, n_rows, n_acc, seed))
    return out


def synth_rows_device(d_ptr: int, first_row: int, n_rows: int, n_acc: int, seed: int, stream: int = 0):
    check(lib.kgwas_synth_rows_device(C.c_void_p(d_ptr), first_row, n_rows, n_acc, seed, C.c_void_p(stream)))


def table_to_bed(out_base: str, table: KmersTable, col, acc_names: Sequence[str], y, min_count: int, batch_size: int,
                 unique_patterns: bool = False, device: int = 0):
    """kmers_table_to_bed: the MAC-filtered table as PLINK files <out_base>.<i>.{bed,bim,fam}, a new set after every
    batch_size kept k-mers; unique_patterns keeps the first k-mer of each presence/absence pattern.
    Returns (batches, k-mers written)."""
    col = np.ascontiguousarray(col, np.uint64)
    y = np.ascontiguousarray(y, np.float32)
    arr = (C.c_char_p * len(acc_names))(*[a.encode() for a in acc_names])
    nb, nw = C.c_uint64(0), C.c_uint64(0)
    check(lib.kgwas_table_to_bed(table._h, ptr(col), len(col), arr, ptr(y), min_count, batch_size, 1 if unique_patterns else 0,
                                 out_base.encode(), device, C.byref(nb), C.byref(nw)))
    return nb.value, nw.value


def kmer2bits(word: str) -> int:
    """kmer2bits (src/kmer_general.cpp:260-283): the canonical 2-bit code of a k-mer of 1 to 32 bases, min(code, reverse
    complement); any character but A, C, G, T raises KgwasError (KGWAS_ERR_FORMAT, "Ilegal kmer")."""
    b = word.encode()
    out = C.c_uint64(0)
    check(lib.kgwas_kmer_encode(b, len(b), C.byref(out)))
    return out.value


def filter_kmers(table: KmersTable, codes, device: int = 0):
    """filter_kmers (src/filter_kmers.cpp) on the GPU: the rows the reference's merge-join of the sorted codes with the
    table emits, in file order. Returns (file_rows uint64[m], rows uint64[m, 1 + W_f])."""
    codes = np.ascontiguousarray(codes, np.uint64).reshape(-1)
    cap = min(len(codes), table.n_rows)
    file_rows = np.zeros(max(cap, 1), np.uint64)
    rows = np.zeros((max(cap, 1), 1 + table.words_per_row), np.uint64)
    m = C.c_uint64(0)
    check(lib.kgwas_filter_kmers(table._h, ptr(codes), len(codes), device, ptr(file_rows), ptr(rows), C.byref(m)))
    return file_rows[:m.value].copy(), rows[:m.value].copy()


def r2_millionths(r2) -> int:
    """The r2 threshold as integer millionths. Text ("0.8") is read digit by digit by the library; a number goes through its
    shortest decimal text (repr), so 0.8 is 800000 and never 799999."""
    text = r2 if isinstance(r2, str) else np.format_float_positional(float(r2), trim="-")
    out = C.c_uint32(0)
    check(lib.kgwas_r2_millionths(text.encode(), C.byref(out)))
    return out.value


def kmers_ld(bits, n_acc: int, r2, tile_rows: int = 0, device: int = 0):
    """Which pairs of presence/absence rows have r^2 >= r2, exactly (kgwas_kmers_ld: the counts of common accessions on the
    matrix cores, the decision in 128-bit integers). bits: uint64[n_kmers, words], bit i of a row = accession i; bits at or
    past n_acc are ignored. Returns (adj uint32[n_kmers, ceil(n_kmers / 32)], n1 uint32[n_kmers]): adj[a, b // 32] bit b % 32
    is set iff b > a and the pair is linked - the upper triangle; the rest is zero."""
    bits = np.ascontiguousarray(bits, np.uint64)
    if bits.ndim != 2:
        raise ValueError("bits must be a 2-d array of uint64 words")
    n_kmers, words = bits.shape
    adj = np.zeros((n_kmers, (n_kmers + 31) // 32), np.uint32)
    n1 = np.zeros(n_kmers, np.uint32)
    check(lib.kgwas_kmers_ld(ptr(bits), n_kmers, words, n_acc, r2_millionths(r2), device, tile_rows, ptr(adj), ptr(n1)))
    return adj, n1


PROXY_RECORD = np.dtype([("row", np.uint64), ("kmer", np.uint64), ("lead", np.uint32), ("n1", np.uint32), ("n11", np.uint32), ("pad", np.uint32)])


def kmers_ld_proxies(lead_bits, bits, n_acc: int, r2, cap: int | None = None, device: int = 0):
    """Which rows of `bits` have r^2 >= r2 with which rows of `lead_bits`, exactly (kgwas_kmers_ld_proxies: the leads stay on the
    device, the rows pass in pieces, the linked pairs come back as records). lead_bits: uint64[n_leads, words], bits:
    uint64[n_rows, words], bit i of a row = accession i; bits at or past n_acc are ignored. Returns (records, n): records is a
    structured array of dtype PROXY_RECORD (row, kmer = 0, lead, n1 of the row, n11, pad = 0) in (row, lead) order and n the count
    of all linked pairs. cap=None: every record is returned (a second call where the first guess was too small); otherwise the
    first min(cap, n)."""
    lead_bits, bits = np.ascontiguousarray(lead_bits, np.uint64), np.ascontiguousarray(bits, np.uint64)
    if lead_bits.ndim != 2 or bits.ndim != 2 or lead_bits.shape[1] != bits.shape[1]:
        raise ValueError("lead_bits and bits must be 2-d arrays of uint64 words with rows of the same width")
    tm, n = r2_millionths(r2), C.c_uint64(0)
    room = (4 * len(bits) + 1024) if cap is None else cap
    while True:
        rec = np.zeros(room, PROXY_RECORD)
        check(lib.kgwas_kmers_ld_proxies(ptr(lead_bits), len(lead_bits), ptr(bits), len(bits), bits.shape[1], n_acc, tm, device,
                                         ptr(rec) if room else None, room, C.byref(n)))
        if cap is not None or n.value <= room:
            return rec[:min(n.value, room)], n.value
        room = n.value


LOCATE_RECORD = np.dtype([("pos", np.uint64), ("kmer", np.uint32), ("strand", np.uint8), ("mismatches", np.uint8), ("offset", np.uint8), ("pad", np.uint8)])


def kmer_codes(kmers, kmer_len: int) -> np.ndarray:
    """The codes of k-mers as spelled (A=0, C=1, G=2, T=3, first base most significant; not the canonical form): what
    locate_kmers_bases takes."""
    out = np.zeros(len(kmers), np.uint64)
    for i, w in enumerate(kmers):
        if len(w) != kmer_len or set(w) - set("ACGT"):
            raise ValueError("kmer_codes: %r is not %d letters of A, C, G, T" % (w, kmer_len))
        c = 0
        for ch in w:
            c = c << 2 | "ACGT".index(ch)
        out[i] = c
    return out


def locate_kmers_bases(bases, codes, kmer_len: int, mismatches: int = 1, cap: int | None = None, device: int = 0):
    """Where in a base stream the k-mers `codes` (uint64, the letters as spelled: kmer_codes), or their reverse complements, occur
    with at most `mismatches` (0 or 1) differing bases (kgwas_locate_kmers_bases: the sorted patterns stay on the device, the stream
    passes in pieces, the hits come back as records). `bases` is bytes, a uint8 NumPy array, or a uint8 torch tensor on the host or
    on `device`: every byte other than A, C, G, T (either case) separates. Returns (records, n): records is a structured array of
    dtype LOCATE_RECORD (pos, kmer, strand, mismatches, offset, pad = 0) in (pos, kmer, strand) order and n the count of all hits.
    cap=None: every record is returned (a second call where the first guess was too small); otherwise the first min(cap, n)."""
    codes = np.ascontiguousarray(codes, np.uint64).reshape(-1)
    on_device = 0
    if hasattr(bases, "data_ptr"):  # a torch tensor
        import torch
        if bases.dtype != torch.uint8:
            raise TypeError("locate_kmers_bases: the bases must be uint8")
        keep = bases.contiguous()
        if keep.is_cuda:
            if keep.device.index != device:
                raise ValueError("locate_kmers_bases: the tensor is on device %s, the search runs on device %d" % (keep.device.index, device))
            torch.cuda.synchronize(keep.device)
            on_device = 1
        p, size = C.c_void_p(keep.data_ptr()), keep.numel()
    elif isinstance(bases, (bytes, bytearray, memoryview, np.ndarray)):
        keep = np.ascontiguousarray(np.frombuffer(bases, np.uint8) if not isinstance(bases, np.ndarray) else bases)
        if keep.dtype != np.uint8:
            raise TypeError("locate_kmers_bases: the bases must be uint8")
        p, size = ptr(keep), keep.size
    else:
        raise TypeError("locate_kmers_bases: bytes, a uint8 array or a uint8 tensor, not %s" % type(bases).__name__)
    n = C.c_uint64(0)
    room = 4096 if cap is None else cap
    while True:
        rec = np.zeros(room, LOCATE_RECORD)
        check(lib.kgwas_locate_kmers_bases(p if size else None, size, on_device, ptr(codes), len(codes), kmer_len, mismatches, device,
                                           ptr(rec) if room else None, room, C.byref(n)))
        if cap is not None or n.value <= room:
            return rec[:min(n.value, room)], n.value
        room = n.value


FETCH_RECORD = np.dtype([("read", np.uint64), ("n_hits", np.uint32), ("first_pos", np.uint32), ("kmer", np.uint32), ("strand", np.uint8), ("pad", np.uint8, (3,))])


def fetch_reads_bases(bases, codes, kmer_len: int, min_hits: int = 1, cap: int | None = None, device: int = 0):
    """The reads of a stream that contain the k-mers `codes` (uint64, the letters as spelled: kmer_codes) or their reverse
    complements (kgwas_fetch_reads_bases). `bases` is bytes or a uint8 NumPy array on the host: a read is the bytes between one
    newline and the next, A C G T (either case) are bases, every other byte breaks windows. Returns (records, n, kmer_windows):
    records is a structured array of dtype FETCH_RECORD (read, n_hits, first_pos, kmer, strand, pad = 0), one per read with at least
    `min_hits` hit windows, in ascending read; n the count of all records; kmer_windows[i] the hit windows of query i over all reads.
    cap=None: every record is returned (a second call where the first guess was too small); otherwise the first min(cap, n)."""
    codes = np.ascontiguousarray(codes, np.uint64).reshape(-1)
    if not isinstance(bases, (bytes, bytearray, memoryview, np.ndarray)):
        raise TypeError("fetch_reads_bases: bytes or a uint8 array, not %s" % type(bases).__name__)
    keep = np.ascontiguousarray(np.frombuffer(bases, np.uint8) if not isinstance(bases, np.ndarray) else bases)
    if keep.dtype != np.uint8:
        raise TypeError("fetch_reads_bases: the bases must be uint8")
    n = C.c_uint64(0)
    room = 4096 if cap is None else cap
    while True:
        rec = np.zeros(room, FETCH_RECORD)
        windows = np.zeros(len(codes), np.uint64)
        check(lib.kgwas_fetch_reads_bases(ptr(keep) if keep.size else None, keep.size, ptr(codes), len(codes), kmer_len, min_hits, device,
                                          ptr(rec) if room else None, room, C.byref(n), ptr(windows) if len(codes) else None))
        if cap is not None or n.value <= room:
            return rec[:min(n.value, room)], n.value, windows
        room = n.value


def fetch_reads(reads_path: str, kmers_path: str, kmer_len: int, out_prefix: str, mates_path: str | None = None, min_hits: int = 1,
                max_reads_per_kmer: int = 0, device: int = 0) -> dict:
    """fetch_reads, the tool (kgwas_fetch_reads_run): the reads of `reads_path` (FASTQ or FASTA; with `mates_path` pairs) that hold
    at least `min_hits` windows spelling a k-mer of `kmers_path` go to out_prefix.fastq / .fasta (out_prefix_1.*, _2.* with mates),
    out_prefix.reads.tsv and out_prefix.log.txt. Returns kgwas_fetch_stats as a dict."""
    st = capi.FetchStats()
    check(lib.kgwas_fetch_reads_run(os.fsencode(reads_path), None if mates_path is None else os.fsencode(mates_path), os.fsencode(kmers_path), kmer_len,
                                    min_hits, max_reads_per_kmer, device, os.fsencode(out_prefix), C.byref(st)))
    return st.as_dict()


def filter_kmers_write(path: str, table: KmersTable, codes, device: int = 0) -> int:
    """filter_kmers' output file for `codes` (header, then one text line per emitted row). Returns the rows written."""
    codes = np.ascontiguousarray(codes, np.uint64).reshape(-1)
    m = C.c_uint64(0)
    check(lib.kgwas_filter_kmers_write(table._h, ptr(codes), len(codes), device, path.encode(), C.byref(m)))
    return m.value


def build_kmers_table(all_kmers_path: str, kmer_paths: Sequence[str], names: Sequence[str] | None, kmer_len: int, out_base: str,
                      device: int = 0) -> int:
    """build_kmers_table (src/build_kmers_table.cpp) on the GPU: writes out_base.table from the sorted all-k-mers file and the
    accessions' sorted k-mer files (64-bit words), and out_base.names when `names` is given. Returns the rows written."""
    paths = (C.c_char_p * len(kmer_paths))(*[os.fsencode(p) for p in kmer_paths])
    nm = None
    if names is not None:
        if len(names) != len(kmer_paths):
            raise ValueError("build_kmers_table: %d names for %d files" % (len(names), len(kmer_paths)))
        nm = (C.c_char_p * len(names))(*[a.encode() for a in names])
    m = C.c_uint64(0)
    check(lib.kgwas_build_table(os.fsencode(all_kmers_path), paths, nm, len(kmer_paths), kmer_len, device, os.fsencode(out_base), C.byref(m)))
    return m.value


def list_kmers_found_in_multiple_samples(kmer_paths: Sequence[str], kmer_len: int, mac: int, min_strand_percent: float, out_path: str,
                                         device: int = 0) -> tuple[int, int, int]:
    """list_kmers_found_in_multiple_samples (src/list_kmers_found_in_multiple_samples.cpp) on the GPU: from the accessions' sorted
    k-mer files (64-bit words, the top two bits a strand flag) writes out_path (the keys found in at least `mac` files and on both
    strands in at least min_strand_percent of them) and out_path.no_pass_kmers / .shareness / .stats.*. Returns the numbers of keys
    that passed, that reached mac but failed the strand rule, and that stayed below mac."""
    paths = (C.c_char_p * len(kmer_paths))(*[os.fsencode(p) for p in kmer_paths])
    counts = (C.c_uint64 * 3)()
    check(lib.kgwas_list_kmers(paths, len(kmer_paths), kmer_len, mac, float(min_strand_percent), device, os.fsencode(out_path), counts))
    return counts[0], counts[1], counts[2]


def count_kmers(reads, kmer_len: int, ci: int, cx: int, out_path: str, device: int = 0) -> tuple[int, ...]:
    """count_kmers_with_strand on the GPU: writes the accession's sorted k-mer file out_path (key | strand flags of the canonical
    k-mers counted ci..cx times, ascending) from its reads and returns the eight counters of kgwas_count_kmers_files (kept keys,
    distinct oriented k-mers, those whose key is kept, kept keys by flag 0..3, counted windows). `reads` is a path or a sequence of
    paths of FASTA / FASTQ files ("-": standard input), or the bases themselves - bytes, a uint8 NumPy array, or a uint8 torch
    tensor on the host or on `device` - as one stream in which every byte other than A, C, G, T separates reads."""
    counts = (C.c_uint64 * 8)()
    out = os.fsencode(out_path)
    if isinstance(reads, (str, os.PathLike)):
        reads = [reads]
    if isinstance(reads, (list, tuple)):
        paths = (C.c_char_p * len(reads))(*[os.fsencode(p) for p in reads])
        check(lib.kgwas_count_kmers_files(paths, len(reads), kmer_len, ci, cx, device, out, counts))
    elif isinstance(reads, (bytes, bytearray, memoryview, np.ndarray)):
        a = np.ascontiguousarray(np.frombuffer(reads, np.uint8) if not isinstance(reads, np.ndarray) else reads)
        if a.dtype != np.uint8:
            raise TypeError("count_kmers: the bases must be uint8")
        check(lib.kgwas_count_kmers_bases(ptr(a), a.size, 0, kmer_len, ci, cx, device, out, counts))
    elif hasattr(reads, "data_ptr"):  # a torch tensor
        import torch
        if reads.dtype != torch.uint8:
            raise TypeError("count_kmers: the bases must be uint8")
        t = reads.contiguous()
        if t.is_cuda:
            if t.device.index != device:
                raise ValueError("count_kmers: the tensor is on device %s, the count runs on device %d" % (t.device.index, device))
            torch.cuda.synchronize(t.device)
        check(lib.kgwas_count_kmers_bases(C.c_void_p(t.data_ptr()), t.numel(), 1 if t.is_cuda else 0, kmer_len, ci, cx, device, out, counts))
    else:
        raise TypeError("count_kmers: paths, bytes, a uint8 array or a uint8 tensor, not %s" % type(reads).__name__)
    return tuple(counts)


class SnpsDataBase:
    """MultipleSNPsDataBases (src/snps_multiple_databases.h:25-63): a PLINK bed/bim/fam trio restricted to the
    phenotyped samples (phenotype order); scoring runs on the GPU."""

    def __init__(self, base_bedbim: str, samples: Sequence[str]):
        self._h = C.c_void_p()
        self.samples = list(samples)
        arr = (C.c_char_p * len(self.samples))(*[a.encode() for a in self.samples])
        check(lib.kgwas_snps_open(base_bedbim.encode(), arr, len(self.samples), C.byref(self._h)))
        n, f, b = C.c_uint64(), C.c_uint64(), C.c_uint64()
        check(lib.kgwas_snps_info(self._h, C.byref(n), C.byref(f), C.byref(b)))
        self.n_snps, self.n_samples_file, self.bytes_per_snp = n.value, f.value, b.value

    def scores(self, Y: np.ndarray, mac: float, device: int = 0) -> np.ndarray:
        """calculate_grammmar_approx_association of every SNP for every row of Y[n_pheno][n_samples]."""
        Y = np.ascontiguousarray(np.atleast_2d(Y), np.float32)
        out = np.zeros((Y.shape[0], self.n_snps), np.float64)
        check(lib.kgwas_snps_scores(self._h, ptr(Y), Y.shape[0], float(mac), device, ptr(out)))
        return out

    def best(self, Y: np.ndarray, topn: int, mac: float, device: int = 0):
        """get_most_associated_snps per phenotype column: list of sorted SNP index arrays."""
        Y = np.ascontiguousarray(np.atleast_2d(Y), np.float32)
        P = Y.shape[0]
        counts = np.zeros(P, np.uint64)
        idx = np.zeros((P, max(topn, 1)), np.uint64)
        check(lib.kgwas_snps_best(self._h, ptr(Y), P, topn, float(mac), device, ptr(counts), ptr(idx)))
        return [idx[j, : int(counts[j])].copy() for j in range(P)]

    def write(self, out_bases: Sequence[str], index_lists):
        """output_plink_bed_file: list l (sorted SNP indices) -> out_bases[l].bed/.bim."""
        n = len(out_bases)
        stride = max([len(x) for x in index_lists] + [1])
        counts = np.asarray([len(x) for x in index_lists], np.uint64)
        idx = np.zeros((n, stride), np.uint64)
        for l, x in enumerate(index_lists):
            idx[l, : len(x)] = x
        arr = (C.c_char_p * n)(*[b.encode() for b in out_bases])
        check(lib.kgwas_snps_write(self._h, n, arr, ptr(counts), ptr(idx), stride))

    def close(self):
        if self._h:
            lib.kgwas_snps_close(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SnpKinship:
    """emma_kinship (src/emma_kinship.cpp): the EMMA kinship of <base>.bed / <base>.fam, accumulated on the GPU with the
    reference's rounding (bit-identical sums). Opening runs the reference's file guards before the device is touched."""

    def __init__(self, base_bedbim: str, device: int = 0):
        self._h = C.c_void_p()
        check(lib.kgwas_snpkin_open(base_bedbim.encode(), device, C.byref(self._h)))
        S, M, b = C.c_uint64(), C.c_uint64(), C.c_uint64()
        check(lib.kgwas_snpkin_info(self._h, C.byref(S), C.byref(M), C.byref(b)))
        self.n_samples, self.n_snps, self.bytes_per_snp = S.value, M.value, b.value

    def feed_bed(self, body):
        """SNPs of a .bed body (file layout, without the 3 magic bytes), after those fed before."""
        body = np.ascontiguousarray(np.frombuffer(body, np.uint8) if isinstance(body, (bytes, bytearray, memoryview)) else body, np.uint8)
        if body.size % self.bytes_per_snp:
            raise ValueError("feed_bed: %d bytes are not whole SNPs of %d bytes" % (body.size, self.bytes_per_snp))
        check(lib.kgwas_snpkin_feed_bed(self._h, ptr(body), body.size // self.bytes_per_snp))

    def feed_file(self):
        """The whole .bed, streamed."""
        check(lib.kgwas_snpkin_feed_file(self._h))

    def sums(self):
        """(undivided sums: [r, c] for c < r, other entries 0; SNPs used)."""
        out = np.zeros((self.n_samples, self.n_samples), np.float64)
        n = C.c_uint64()
        check(lib.kgwas_snpkin_sums(self._h, ptr(out), C.byref(n)))
        return out, n.value

    def matrix(self):
        """(the finished S x S kinship matrix, SNPs used)."""
        K = np.zeros((self.n_samples, self.n_samples), np.float64)
        n = C.c_uint64()
        check(lib.kgwas_snpkin_matrix(self._h, ptr(K), C.byref(n)))
        return K, n.value

    def close(self):
        if self._h:
            lib.kgwas_snpkin_close(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def snp_kinship_format(K: np.ndarray) -> bytes:
    """The text emma_kinship prints for the matrix K."""
    K = np.ascontiguousarray(K, np.float64)
    need = lib.kgwas_snpkin_format(K.shape[0], ptr(K), None, 0)
    buf = C.create_string_buffer(int(need) + 1)
    lib.kgwas_snpkin_format(K.shape[0], ptr(K), buf, need)
    return buf.raw[:need]
