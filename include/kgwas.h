/* include/kgwas.h — C ABI of libkgwas: the MI355X-native k-mer association-scan engine.
 *
 * Drop-in boundary for ONE hot path of voichek/kmersGWAS: the associate_kmers /
 * emma_kinship_kmers scan. The reference has no plugin or FFI interface — its boundary is
 * the process (argv + files) and, inside the binary, the method surface of
 * MultipleKmersDataBases and BestAssociationsHeap. Each entry point below names the
 * reference interface it replaces (paths relative to the reference tree).
 *
 * Conventions: plain C, no exceptions cross the boundary. Every function returns
 * KGWAS_OK (0) or a negative KGWAS_ERR_*; kgwas_last_error() gives the thread-local
 * message. Handles are created and freed by the library. Caller-owned input buffers are
 * only read during the call. Result pointers stay valid until the owning handle is
 * destroyed. All compute runs on the GPU through hand-written gfx950 kernels: there is
 * NO CPU fallback — without a usable HIP device the compute entry points fail with
 * KGWAS_ERR_DEVICE.
 */
#ifndef KGWAS_H
#define KGWAS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KGWAS_OK 0
#define KGWAS_ERR_ARG (-1)    /* bad argument */
#define KGWAS_ERR_IO (-2)     /* file cannot be opened / read / written */
#define KGWAS_ERR_FORMAT (-3) /* a reference std::logic_error: bad magic, k, size, unknown accession ... */
#define KGWAS_ERR_DEVICE (-4) /* no HIP device or a HIP call failed */
#define KGWAS_ERR_STATE (-5)  /* call out of order */
#define KGWAS_ERR_NOMEM (-6)

const char* kgwas_last_error(void);
int kgwas_version(void);
int kgwas_device_count(int* n_devices);
/* CPUs this process may really keep busy: the cgroup CPU quota if there is one, else the hardware thread count. What
 * kgwas_scan_params.host_threads = 0 resolves to; the command-line tools raise a smaller --parallel to it (the
 * reference's --parallel sizes a pool of scoring tasks, kmers_gwas.py passes 1 by default - pipeline_parser.py:31 -
 * and here the threads replay heap pushes beside the GPU: one thread would be ~20x slower than the GPU it serves). */
uint32_t kgwas_host_cpu_quota(void);

/* ------------------------------------------------------------------------------------
 * .table / .names reader.
 * Replaces MultipleKmersDataBases::MultipleKmersDataBases header guards
 * (src/kmers_multiple_databases.cpp:39-94), load_kmers_talbe_column_names
 * (src/kmer_general.cpp:45-53) and create_map_from_all_DBs (:297-311).
 * kmer_len == 0 skips the k check (for tools that do not know k).
 * ---------------------------------------------------------------------------------- */
typedef struct kgwas_table kgwas_table;
int kgwas_table_open(const char* base, uint32_t kmer_len, kgwas_table** out);
int kgwas_table_info(const kgwas_table* t, uint64_t* n_acc_file, uint64_t* n_rows, uint64_t* words_per_row,
                     uint32_t* kmer_len);
int kgwas_table_name(const kgwas_table* t, uint64_t i, const char** name);
/* col_out[i] = file column of accession acc[i]; unknown or duplicated name -> KGWAS_ERR_FORMAT
 * (intersect_phenotypes_to_present_DBs with must_be_present, src/kmer_general.cpp:239-253;
 *  get_index_DB :227-237). */
int kgwas_table_column_map(const kgwas_table* t, const char* const* acc, uint64_t n, uint64_t* col_out);
/* Raw rows [u64 kmer][W_f u64] of file rows [row0, row0+n) into dst (host). */
int kgwas_table_read_rows(kgwas_table* t, uint64_t row0, uint64_t n, uint64_t* dst);
void kgwas_table_close(kgwas_table* t);

/* ------------------------------------------------------------------------------------
 * Phenotype TSV. Replaces load_phenotypes_file (src/kmer_general.cpp:175-205).
 * ---------------------------------------------------------------------------------- */
typedef struct kgwas_pheno kgwas_pheno;
int kgwas_pheno_load(const char* path, kgwas_pheno** out);
int kgwas_pheno_info(const kgwas_pheno* p, uint64_t* n_pheno, uint64_t* n_acc);
int kgwas_pheno_name(const kgwas_pheno* p, uint64_t j, const char** name);
int kgwas_pheno_accession(const kgwas_pheno* p, uint64_t i, const char** acc);
/* Y: n_pheno x n_acc float32, row-major, accession (file) order of the TSV. */
int kgwas_pheno_values(const kgwas_pheno* p, const float** Y);
void kgwas_pheno_free(kgwas_pheno* p);

/* min_count = max(ceil(n_acc*maf), mac) (src/associate_kmers.cpp:99-103). */
uint64_t kgwas_min_count(uint64_t n_acc, double maf, uint64_t mac);

/* ------------------------------------------------------------------------------------
 * BestAssociationsHeap (src/best_associations_heap.h:32-54, .cpp:26-127): bounded min-heap
 * with the reference's strict-'>' replacement. NOT a std::priority_queue: csrc/heap.h performs,
 * by hand, the element moves libstdc++'s std::push_heap / std::pop_heap (__push_heap, __adjust_heap)
 * make for the reference's comparator (a.score > b.score, src/kmer_general.h:113-128) - on 16-byte
 * (score, slot) entries, several heaps in lockstep, integer compares where all scores are >= +0 -
 * so that ties resolve identically: which equal-score entry survives at the boundary and the order
 * equal scores pop in. The emulation is pinned against a literal std::priority_queue over the
 * reference's tuple type (oracle/oracle.cpp) on tie-heavy, NaN, negative and +inf streams, in the
 * CPU suite (tests/test_host.py::test_heap_mirror_equals_oracle_heap_under_ties) and again on the
 * GPU box (tests/test_gpu_parity.py::test_heap_mirror_equals_std_priority_queue_on_the_gpu_box);
 * checked against libstdc++ of GCC 11.4 (GLIBCXX_3.4.30), the toolchain of this image and of the
 * test boxes. A libstdc++ whose heap algorithms move elements differently would fail those tests;
 * the reference itself would then produce different tie orders with it.
 * Used by the scan for its host-side replay and exposed for cross-shard merges.
 * RUN-TIME GUARD (csrc/heap_guard.cpp): once per process, before the first heap or session exists, a fixed stream of ties, NaNs,
 * negative and infinite scores goes through the emulation (single pushes and the lockstep form) and through a literal
 * std::priority_queue over the reference's tuple / comparator of THE LIBSTDC++ THIS PROCESS RUNS WITH; on any difference
 * kgwas_heap_new, kgwas_scan_create, kgwas_multiscan_create and kgwas_snps_* return KGWAS_ERR_STATE. kgwas_heap_selfcheck(0) runs
 * (or re-reports) that check; kgwas_heap_selfcheck(1) is a test hook that holds the emulation against a reference with a
 * DIFFERENT tie rule and must therefore fail.
 * ---------------------------------------------------------------------------------- */
int kgwas_heap_selfcheck(uint32_t flags);
typedef struct kgwas_heap kgwas_heap;
int kgwas_heap_new(uint64_t max_results, kgwas_heap** out);
/* add_association for n entries in the given order. */
int kgwas_heap_add_many(kgwas_heap* h, const uint64_t* kmer, const double* score, const uint64_t* row, uint64_t n);
int kgwas_heap_size(const kgwas_heap* h, uint64_t* size, uint64_t* insertions, double* lowest);
/* output_to_file_with_scores order: ascending pops from a copy; arrays hold `size` entries. */
int kgwas_heap_pop_all(const kgwas_heap* h, uint64_t* kmer, double* score, uint64_t* row);
/* get_kmers_for_output: (kmer, rank, row) sorted by row; rank = queue size at pop (best = 1). */
int kgwas_heap_output_list(const kgwas_heap* h, uint64_t* kmer, uint64_t* rank, uint64_t* row);
/* get_rows_sorted_indices (src/best_associations_heap.cpp:135-147): the entries' row indices, ascending; `size` entries. */
int kgwas_heap_rows_sorted(const kgwas_heap* h, uint64_t* row);
/* output_to_file (:65-74, with_scores = 0: the k-mers as 8 bytes each) / output_to_file_with_scores (:80-90, with_scores = 1:
 * k-mer + score, 16 bytes each), in ascending pop order; the file is created or truncated. */
int kgwas_heap_output_to_file(const kgwas_heap* h, const char* path, int with_scores);
void kgwas_heap_free(kgwas_heap* h);

/* Test hook: one phenotype column's select-or-replay decision on the host alone (scan_lazy.cpp). The records
 * of n_chunks chunks (chunk c: chunk_n[c] records, rows chunk_row0[c] + row_in_chunk[i], ascending; a score of -inf is a
 * placeholder and no record) are logged - by reference into the caller's arrays (by_ref != 0) or by copy, the logs detached from
 * the caller's arrays behind chunk `detach_after_chunk` (< 0: never) - with chunk_thr[c] as the device's threshold behind chunk c
 * (any lower bound of the N-th largest score up to there; 0: none). Then the column is finished: *selected = 1 if its N + 1
 * largest scores were pairwise distinct, none NaN or negative, and the lists were made by selection; 0 if its log was replayed
 * through the heap mirror. out_*: the result lists in ascending pop order (room for topn entries), *out_n their length. */
int kgwas_select_check(uint64_t topn, uint64_t n_chunks, const uint64_t* chunk_n, const uint64_t* chunk_row0, const double* chunk_thr,
                       const double* score, const uint64_t* kmer, const uint32_t* row_in_chunk, int by_ref, int64_t detach_after_chunk,
                       int* selected, uint64_t* out_kmer, double* out_score, uint64_t* out_row, uint64_t* out_n);

/* ------------------------------------------------------------------------------------
 * Association scan session = pass 1 of associate_kmers (src/associate_kmers.cpp:99-148):
 * MultipleKmersDataBases::load_kmers (MAC filter + squeeze, :103-146),
 * add_kmers_to_heap / calculate_kmer_score (:275-284, :327-363) for every phenotype column,
 * feeding one BestAssociationsHeap per column. Rows are fed in file order, in any number of
 * feed calls; results do not depend on how the rows are split.
 * ---------------------------------------------------------------------------------- */
typedef struct kgwas_scan kgwas_scan;

#define KGWAS_KERNEL_AUTO 0
#define KGWAS_KERNEL_VALU 1 /* exact-order select+add on the vector ALU */
#define KGWAS_KERNEL_MFMA 2 /* exact-order f32 MFMA (v_mfma_f32_16x16x4_f32) */
#define KGWAS_KERNEL_COARSE 3 /* matrix-pipe coarse filter (block-scaled FP4 x FP6/FP4, or int8 with KGWAS_COARSE_MX=0) with a rigorous bound + exact re-scoring of survivors;
                                the dense phase and overflow re-runs use an exact kernel. Same results. */
#define KGWAS_KERNEL_NARROW 4 /* reported in kgwas_scan_stats.kernel_used only: the filter of scans with 1-4 phenotype
                                columns (FP4 table bits x FP8 phenotype slices on the block-scaled MFMA; requested
                                through KGWAS_KERNEL_AUTO or _COARSE), exact re-scoring as above. Same results. */

typedef struct kgwas_scan_params {
    uint32_t struct_size;    /* sizeof(kgwas_scan_params) */
    int32_t device;          /* HIP device ordinal */
    uint64_t n_acc_file;     /* S_f: accessions (bit columns) in the table */
    uint64_t n_acc;          /* S: phenotyped accessions */
    const uint64_t* col;     /* [S] file column of phenotyped accession i (phenotype order) */
    uint64_t n_pheno;        /* phenotype columns (1 + permutations) */
    const float* Y;          /* n_pheno x S float32 row-major, phenotype order */
    const uint64_t* topn;    /* [n_pheno] heap sizes (-n / --first_phenotype_best) */
    uint64_t min_count;      /* effective minor allele count */
    uint64_t chunk_rows;     /* max rows per device chunk; 0 = default */
    uint32_t host_threads;   /* replay threads; 0 = hardware concurrency */
    uint32_t kernel;         /* KGWAS_KERNEL_* */
    uint32_t record_history; /* what a later shard must keep for a cross-shard merge: 1 = every effective heap push
                                (kgwas_scan_history, kgwas_scan_history_above); 2 = only each heap's last evictions
                                (kgwas_scan_history_above alone; it fails loudly if the ring was too short) */
    uint32_t count_patterns; /* --pattern_counter: count distinct presence/absence patterns of tested rows */
} kgwas_scan_params;

typedef struct kgwas_scan_stats {
    uint64_t rows_fed;          /* file rows seen */
    uint64_t rows_tested;       /* rows passing the MAC filter (= .tested_kmers) */
    uint64_t candidates;        /* (row, phenotype) records shipped device -> host */
    uint64_t heap_pushes;       /* effective pushes over all heaps */
    uint64_t chunks;            /* device chunks launched */
    uint64_t score_launches;    /* launches of the scoring kernel */
    double score_kernel_ms;     /* sum of hipEvent durations of the scoring kernel */
    double squeeze_kernel_ms;   /* sum of hipEvent durations of the squeeze kernel (0 in direct mode) */
    double replay_ms;           /* host time spent replaying candidates: the busiest replay worker's busy time (the workers
                                   run beside the GPU and beside each other) + the synchronous dense / overflow replays */
    double gpu_wait_ms;         /* host wall time blocked waiting for sparse chunks to finish */
    double dense_ms;            /* host wall time of the dense (heap-filling) phase, GPU + replay */
    double coarse_kernel_ms;    /* sum of hipEvent durations of coarse_kernel alone (KGWAS_KERNEL_COARSE) */
    uint64_t coarse_launches;   /* its launches */
    uint32_t kernel_used;       /* KGWAS_KERNEL_VALU, _MFMA, _COARSE or _NARROW */
    uint32_t direct_mode;       /* 1 = scorer read the file layout in place (no squeeze pass) */
    uint64_t patterns;          /* distinct pattern hashes among tested rows (count_patterns; valid after finish) */
    /* coarse filter, per operand set: [0] = one int8 slice per phenotype column, [1] = two slices */
    uint32_t coarse_mode_tiles[2];     /* 16-column int8 operand tiles per LDS group of the set's main launch (0 = set not built) */
    uint32_t coarse_mode_lgroups[2];   /* LDS groups a row passes through (all launches of the set) */
    uint64_t coarse_mode_launches[2];
    uint64_t coarse_mode_rows[2];      /* rows filtered with this set */
    double coarse_mode_ms[2];          /* hipEvent time of its coarse_kernel launches */
    double replay_cpu_ms;       /* CPU time of the replay summed over the workers (replay_ms: the busiest worker's share) */
    double replay_tail_ms;      /* wall time the replay still needed after the GPU had finished the feed's last chunk */
    uint32_t coarse_mode_tile_slices[2]; /* operand tiles a row is multiplied with, over all LDS groups and launches of the set */
    uint32_t coarse_mx;         /* 1 = the filter is the block-scaled one (score_mx.hip: FP4 table bits x FP6 / FP4 slices on
                                   v_mfma_scale_f32_16x16x128_f8f6f4; coarse_mode_tiles then counts COLUMN tiles, each carrying
                                   all slices of its 16 columns), 0 = the int8 one (KGWAS_COARSE_MX=0) */
    uint32_t coarse_mx_s1_fp6;  /* block-scaled filter: the second slice is FP6 (else FP4) */
    uint32_t coarse_mx_steps;   /* block-scaled filter: MFMA steps (K = 128) per row tile, column tile and slice */
    uint32_t replay_threads;    /* host threads replaying heap pushes in this session */
    double replay_min_ms;       /* the LEAST busy replay worker's busy time (replay_ms: the busiest one's; replay_cpu_ms / replay_threads: the mean) */
    double replay_wall_ms;      /* wall time from the start of the streaming replay (first sparse chunk submitted) to its end */
    uint64_t replay_splits;     /* column groups of the replay that left their worker because they had fallen behind (a slow or
                                   shared CPU under it): handed whole to the workers that are ahead, or cut into single
                                   columns once other workers had nothing left to do */
    uint64_t columns_popped_ahead; /* columns whose result lists were made by idle replay workers at the end of the last feed
                                      (kgwas_scan_expect_finish) instead of by kgwas_scan_finish */
    uint32_t coarse_mx32;       /* always 0 since round 6: the 32 x 32 x 64 form of the block-scaled filter (built, verified and measured
                                   slower in round 4: docs/HISTORY.md) was removed; the field keeps the struct's layout */
    uint32_t coarse_mx_stream;  /* block-scaled filter in its operand-streaming form (score_mxs.hip: all column tiles of an operand
                                   group per wave, operands through an LDS ring; every row loaded and expanded once per group):
                                   1 = the default shapes (one column group of up to 7 tiles, or two of them side by side in a
                                   block), 2 / 3 = one column group of up to 13 tiles with eight waves of 32 rows / four waves of 64
                                   (KGWAS_MXS_FORM=1 / 2). This field replaces the former `reserved0`: the struct's size and
                                   layout are unchanged. */
    /* -- added in ABI version 5 (kgwas_abi_version): the struct grew by 8 bytes -- */
    uint32_t columns_selected;  /* columns whose result lists kgwas_scan_finish made by SELECTION: their N largest scores (and the
                                   N + 1-th) were pairwise distinct, none NaN or negative, so the lists are the N largest in ascending
                                   order whatever libstdc++'s heap layout; such columns' candidates were logged, not replayed, and
                                   heap_pushes does not count them (KGWAS_FULL_REPLAY=1: every column is replayed, as before) */
    uint32_t columns_replayed_at_finish; /* columns that were in select mode until finish and then needed the exact replay of their
                                   log (a tie among their N + 1 largest scores that did not show in the first dense chunk) */
} kgwas_scan_stats;

/* Version of this header's struct layouts and entry points. A caller built against an older header must not pass its (smaller)
 * kgwas_scan_stats to a newer library: compare KGWAS_ABI_VERSION with kgwas_abi_version() at start-up.
 * Version 6 (round 6): no struct changed; new entry points kgwas_heap_selfcheck, kgwas_scan_select_mode and the test hook
 * kgwas_scan_debug_residuals; kgwas_scan_lowest takes a non-const session (it always mutated it); kgwas_scan_stats.coarse_mx32 is
 * always 0 (the 32 x 32 x 64 filter form was removed).
 * Version 7: no struct changed; new entry points kgwas_snpkin_* (emma_kinship).
 * Version 8: no struct changed; new entry points kgwas_kmer_encode, kgwas_filter_kmers, kgwas_filter_kmers_write (filter_kmers).
 * Version 9: no struct changed; new entry point kgwas_build_table (build_kmers_table).
 * Version 10: no struct changed; new entry point kgwas_scan_debug_survivors (test hook).
 * Version 11: no struct changed; new entry point kgwas_list_kmers (list_kmers_found_in_multiple_samples).
 * Version 12: no struct changed; new entry points kgwas_count_kmers_files, kgwas_count_kmers_bases (count_kmers_with_strand).
 * Version 13: no struct changed; new struct kgwas_lmm_stats and entry points kgwas_sym_eigen, kgwas_lmm_* (lmm_lrt).
 * Version 14: no struct changed; new entry points kgwas_lmm_test_bed_multi, kgwas_lmm_run_file_multi (lmm_lrt --columns).
 * Version 15: no struct changed; new entry points kgwas_lmm_test_table, kgwas_lmm_run_table (lmm_lrt --kmers_table), and later,
 * without a new version number, kgwas_lmm_test_table_multi, kgwas_lmm_run_table_multi (lmm_lrt --kmers_table --pheno_columns), and
 * kgwas_lmm_null_reml, kgwas_lmm_test_bed_all, kgwas_lmm_run_files_all, kgwas_lmm_format_assoc4, kgwas_fdist_tail (lmm_lrt -lmm 4),
 * and kgwas_lmm_set_covariates, kgwas_lmm_read_covariates, kgwas_lmm_run_files_cov, kgwas_lmm_run_table_cov (lmm_lrt -c),
 * and struct kgwas_lmm_unique_stats, kgwas_lmm_test_table_unique, kgwas_lmm_run_table_unique (lmm_lrt --pattern_cache),
 * and struct kgwas_lmm_skip_stats, kgwas_lmm_test_table_multi_skip, kgwas_lmm_run_table_multi_skip (lmm_lrt --pattern_skip),
 * and structs kgwas_proxy_record, kgwas_proxy_stats, kgwas_kmers_ld_proxies, kgwas_proxy_kmers_run (proxy_kmers).
 * and structs kgwas_locate_record, kgwas_locate_stats, kgwas_locate_kmers_bases, kgwas_locate_kmers_run (locate_kmers).
 * and structs kgwas_fetch_record, kgwas_fetch_stats, kgwas_fetch_reads_bases, kgwas_fetch_reads_run (fetch_reads).
 * Those came after version 15 without a bump: a caller that may meet an older version-15 library probes for them by symbol
 * (dlsym, or hasattr on a ctypes handle). */
#define KGWAS_ABI_VERSION 15
uint32_t kgwas_abi_version(void);

int kgwas_scan_create(const kgwas_scan_params* p, kgwas_scan** out);
/* A hint, never needed for correctness: the NEXT feed is the last one before kgwas_scan_finish (the tools know it: they
 * feed a whole table). kgwas_scan_finish pops every heap into its result lists (output_to_file_with_scores' order,
 * src/best_associations_heap.cpp:82-92) - 10 001 pops per column; with the hint, replay workers that run out of records
 * near the end of that feed pop the columns that are complete while the slowest worker is still replaying, and finish
 * only does what is left. Anything that changes a heap afterwards (another feed, kgwas_scan_absorb,
 * kgwas_scan_heaps_import) discards those lists. */
int kgwas_scan_expect_finish(kgwas_scan* s);
/* Rows already resident in HBM (file layout, 8-byte aligned). hip_stream may be NULL. */
int kgwas_scan_feed_device(kgwas_scan* s, const void* d_rows, uint64_t n_rows, uint64_t first_row, void* hip_stream);
/* Rows in host memory (file layout). Chunked, double-buffered: a producer thread stages 128 MiB pieces into pinned
 * memory and piece k+1 is copied (own stream) while piece k is scored and replayed. */
int kgwas_scan_feed_host(kgwas_scan* s, const uint64_t* rows, uint64_t n_rows, uint64_t first_row);
/* Rows [row0, row0 + n_rows) straight from an open .table: the same pipeline with the producer thread reading the
 * file (pread) into the pinned pieces, so disk, PCIe and GPU + replay overlap. Replaces the reference's
 * load-a-batch-then-compute loop (src/associate_kmers.cpp:104-148); first_row of the feed is row0. */
int kgwas_scan_feed_table(kgwas_scan* s, kgwas_table* t, uint64_t row0, uint64_t n_rows);
int kgwas_scan_finish(kgwas_scan* s);
/* Heap of phenotype j in heap-pop (ascending score) order: rank of entry i is n - i.
 * row = file row index. Valid after kgwas_scan_finish. */
int kgwas_scan_result(kgwas_scan* s, uint64_t j, uint64_t* n, const uint64_t** kmer, const double** score,
                      const uint64_t** row);
/* Effective pushes of phenotype j in row order (needs record_history). */
int kgwas_scan_history(kgwas_scan* s, uint64_t j, uint64_t* n, const uint64_t** kmer, const double** score,
                       const uint64_t** row);
int kgwas_scan_get_stats(const kgwas_scan* s, kgwas_scan_stats* st);
/* Empty the heaps, histories and statistics but keep every device / pinned buffer, so a session can
 * scan another table (or the same one again) without paying allocation again. */
int kgwas_scan_reset(kgwas_scan* s);
void kgwas_scan_destroy(kgwas_scan* s);

/* Cross-shard merge without re-playing shard 0: current heap minima (lowest_score) and fullness of
 * every column, and in-order replay of later shards' (pre-filtered) histories INTO this scan's heaps.
 * Exactness: the heap of shard 0 is what a single scan holds after those rows; an entry of shard g >= 1
 * whose score is not above max(final minima of the full heaps of shards < g) is rejected by
 * add_association whenever it arrives, so the sender may drop it. counts/kmer/score/row as in
 * kgwas_merge_shards (shards in row order, all after this scan's rows). Call kgwas_scan_finish again.
 * kgwas_scan_lowest MUTATES the session (it is not a read-only query): for columns in select mode it brings their pools up to
 * date and may run a selection, and a column that saw a NaN or negative score is given its heap (its log replayed, heap_pushes
 * grows). It must not overlap a feed or another call on the same session.
 * kgwas_scan_select_mode: *on = 1 if the session keeps its columns in select mode (logs + pools, result lists by selection where
 * the scores decide) - i.e. a filter session without a full push log and without KGWAS_FULL_REPLAY=1 -, 0 if
 * every column is replayed as it streams (exact-scorer sessions among them). Merge layers use it to pick their route. */
int kgwas_scan_lowest(kgwas_scan* s, double* lowest, uint8_t* full);
int kgwas_scan_select_mode(const kgwas_scan* s, int* on);
/* Test hook (sessions created under KGWAS_DEBUG_RESIDUALS=1, else KGWAS_ERR_STATE): the quantisation residuals of column
 * `column` in phenotype-file order - resid_i = y_i - c - (the value the filter form's slices encode for sample i) - for form 0
 * (one-slice operand set), 1 (two-slice set: block-scaled FP6 + FP4 / FP6 + FP6 or int8, whichever the session built) or 2
 * (narrow filter, three FP8 slices). A row whose set bits are exactly the samples with resid_i > 0 attains
 * sum_i g_i resid_i = Rall: the filters' bound |yigi_ref - yc| <= Eg + min(Rall, N1 rmax) is tight there, which is where a test
 * has to look for lost pushes (tests/test_gpu_parity.py::test_adversarial_rows_at_the_filters_bound). */
int kgwas_scan_debug_residuals(const kgwas_scan* s, uint32_t form, uint64_t column, double* out);
/* Test hook (filter sessions created under KGWAS_DEBUG_SURVIVORS=1, else KGWAS_ERR_STATE): what the filter kept, chunk by chunk.
 * Such a session logs every sparse chunk that went through a filter, in submission order: the n_pheno thresholds as that chunk's
 * filter launches read them (a stream-ordered copy of the array the kernels are given, taken behind the chunk's prep launch - the
 * narrow path raises thresholds there - and before its first filter launch) and its survivors. The survivors are taken from the
 * KEY LIST behind the key launch (not from the bitmap in front of it), so the bitmap-to-keys kernels are observed as well and the
 * wide and the narrow path report in one form: (column, row in chunk) pairs in list order - columns ascending, rows ascending
 * within a column; the column is the one the key itself names. The copies are synchronous: the hook serialises the scan; without
 * it a session launches, copies and allocates nothing more than before. kgwas_scan_reset empties the log.
 * *n_chunks (may be NULL): logged chunks. With info, thr or pairs non-NULL, chunk < *n_chunks selects one:
 *   info[0..4] = first_row, n_rows, operand set (0 one-slice, 1 two-slice set - kgwas_scan_stats.coarse_mode_* -, 2 narrow filter),
 *                1 if the key list overflowed (no pairs are logged then; the chunk's re-run by the exact scorer is not logged
 *                either), number of pairs;
 *   thr[n_pheno]; pairs[2 * info[4]] = column, row, column, row, ... (call once for info[4], then with the buffer). */
int kgwas_scan_debug_survivors(const kgwas_scan* s, uint64_t* n_chunks, uint64_t chunk, uint64_t* info, double* thr, uint32_t* pairs);
int kgwas_scan_absorb(kgwas_scan* s, uint64_t n_shards, const uint64_t* counts, const uint64_t* const* kmer,
                      const double* const* score, const uint64_t* const* row);
/* The part of the recorded history that can still matter after heaps whose minima are thr[j]: entries with
 * score > thr[j] (thr[j] = -inf keeps all), column by column, flat: counts[j] entries of column j follow those of
 * column j-1. The arrays stay valid until the next call of this function or of kgwas_scan_heaps_export. */
int kgwas_scan_history_above(kgwas_scan* s, const double* thr, uint64_t* counts, const uint64_t** kmer,
                             const double** score, const uint64_t** row);
/* Column-distributed merge: the state of heaps cols[0..n_cols) in heap-array order (sizes[c] entries each, flat),
 * and its exact re-creation in another scan session of the same shape - layout included, so the heap goes on
 * there exactly as it would have here (a block of columns of a multi-GPU job is merged on one rank). */
int kgwas_scan_heaps_export(kgwas_scan* s, uint64_t n_cols, const uint64_t* cols, uint64_t* sizes, const uint64_t** kmer,
                            const double** score, const uint64_t** row);
int kgwas_scan_heaps_import(kgwas_scan* s, uint64_t n_cols, const uint64_t* cols, const uint64_t* sizes, const uint64_t* kmer,
                            const double* score, const uint64_t* row);
/* The same two exports as MESSAGES written straight into caller memory (the pinned staging buffer of an all-to-all):
 * message m covers the columns msg_col0[m] .. msg_col0[m] + msg_ncols[m] - 1 and is laid out as 64-bit words
 *   [words that follow][counts or sizes: msg_ncols[m]][kmer: T][score bit patterns: T][row: T],  T = sum of the counts
 * (msg_ncols[m] = 0: the one word 0). Messages follow each other in `out`; msg_words[m] receives message m's length.
 * Nothing is written unless the messages fit cap_words (the caller grows the buffer and calls again). */
int kgwas_scan_history_above_msgs(kgwas_scan* s, const double* thr, uint64_t n_msgs, const uint64_t* msg_col0,
                                  const uint64_t* msg_ncols, uint64_t* out, uint64_t cap_words, uint64_t* msg_words);
int kgwas_scan_heaps_export_msgs(kgwas_scan* s, uint64_t n_msgs, const uint64_t* msg_col0, const uint64_t* msg_ncols,
                                 uint64_t* out, uint64_t cap_words, uint64_t* msg_words);

/* ------------------------------------------------------------------------------------
 * The same scan over several GPUs of one node, inside one process (the reference's caller, kmers_gwas.py:133-148, runs
 * ONE associate_kmers binary): the rows are cut into n_devices contiguous shards in file order, shard g is scanned on
 * devices[g] by its own session and host thread (a device may be listed more than once), no data moves between the
 * devices during the scan, and the later shards' effective heap pushes that can still matter are then replayed, in
 * row order, into shard 0's heaps (kgwas_scan_history_above / kgwas_scan_absorb). Results are those of a single scan.
 * p->device is ignored; p->host_threads is the replay-thread budget of the whole job (divided among the shards);
 * p->record_history applies to shard 0 (later shards keep what the merge needs; a shard whose eviction ring turns out
 * too short is scanned again with the full log). kgwas_multiscan_run_* may be called repeatedly with consecutive row
 * ranges (not with count_patterns); call kgwas_multiscan_finish before reading results.
 * ---------------------------------------------------------------------------------- */
typedef struct kgwas_multiscan kgwas_multiscan;
int kgwas_multiscan_create(const kgwas_scan_params* p, const int32_t* devices, uint32_t n_devices, kgwas_multiscan** out);
/* Rows [row0, row0 + n_rows) of an open .table: shard g = the g-th of n_devices equal contiguous pieces, streamed
 * through kgwas_scan_feed_table on its device. */
int kgwas_multiscan_run_table(kgwas_multiscan* m, kgwas_table* t, uint64_t row0, uint64_t n_rows);
/* Shards already resident in HBM: d_rows[g] on devices[g] holds n_rows[g] rows starting at file row first_row[g]
 * (consecutive shards, in row order). */
int kgwas_multiscan_run_device(kgwas_multiscan* m, const void* const* d_rows, const uint64_t* n_rows, const uint64_t* first_row);
int kgwas_multiscan_finish(kgwas_multiscan* m);
/* As kgwas_scan_result, for the whole table. */
int kgwas_multiscan_result(kgwas_multiscan* m, uint64_t j, uint64_t* n, const uint64_t** kmer, const double** score,
                           const uint64_t** row);
/* total: counters summed over the shards (rows_tested = .tested_kmers, patterns over all shards), times of the slowest
 * shard; per_shard [n_devices] (NULL: skip) = each session's own statistics of the last run; scan_ms / merge_ms: wall
 * time of the shard scans and of the cross-shard merges so far; rescans: shards scanned twice (ring too short). */
int kgwas_multiscan_get_stats(const kgwas_multiscan* m, kgwas_scan_stats* total, kgwas_scan_stats* per_shard, double* scan_ms,
                              double* merge_ms, uint64_t* rescans);
void kgwas_multiscan_destroy(kgwas_multiscan* m);

/* calculate_kmer_score for every row and phenotype column (src/kmers_multiple_databases.cpp:327-363):
 * scores[j*n_rows + r] (0 for rows the MAC filter drops), popcnt[r] = masked popcount N1,
 * outputs in host memory. rows_on_device selects how `rows` is interpreted. */
int kgwas_scan_scores_dense(kgwas_scan* s, const void* rows, int rows_on_device, uint64_t n_rows, double* scores,
                            uint32_t* popcnt);

/* Cross-shard merge: replay shard histories (shards in row order) through fresh heaps.
 * counts[g*n_pheno + j] entries of shard g / phenotype j, concatenated by phenotype inside
 * kmer[g] / score[g] / row[g]. Returns one heap per phenotype in out_heaps[j]. */
int kgwas_merge_shards(uint64_t n_pheno, const uint64_t* topn, uint64_t n_shards, const uint64_t* counts,
                       const uint64_t* const* kmer, const double* const* score, const uint64_t* const* row,
                       uint32_t threads, kgwas_heap** out_heaps);

/* ------------------------------------------------------------------------------------
 * Kinship = emma_kinship_kmers (src/emma_kinship_kmers.cpp:77-111) with
 * update_emma_kinshhip_calculation (src/kmers_multiple_databases.cpp:418-438):
 * over rows with min_count <= popcount(all S_f columns) <= S_f - min_count,
 * K[i][j] += 1 ^ g_i ^ g_j for j < i.
 * ---------------------------------------------------------------------------------- */
typedef struct kgwas_kinship kgwas_kinship;
int kgwas_kinship_create(int32_t device, uint64_t n_acc_file, uint64_t min_count, kgwas_kinship** out);
int kgwas_kinship_feed_device(kgwas_kinship* k, const void* d_rows, uint64_t n_rows, void* hip_stream);
int kgwas_kinship_feed_host(kgwas_kinship* k, const uint64_t* rows, uint64_t n_rows);
/* Rows [row0, row0 + n_rows) of an open .table through the double-buffered ingest (file read, copy and kernels
 * overlap); replaces the reference's load-a-batch-then-accumulate loop (src/emma_kinship_kmers.cpp:86-99). */
int kgwas_kinship_feed_table(kgwas_kinship* k, kgwas_table* t, uint64_t row0, uint64_t n_rows);
/* Hamming-distance partials (S_f x S_f u64, full symmetric) and rows used so far: integer, so
 * partials of different shards simply add (all-reduce) before kgwas_kinship_from_partials. */
int kgwas_kinship_partials(kgwas_kinship* k, uint64_t* hamming, uint64_t* n_used);
/* K (S_f x S_f, lower triangle j < i filled like the reference, rest 0) from summed partials. */
int kgwas_kinship_from_partials(uint64_t n_acc_file, const uint64_t* hamming, uint64_t n_used, uint64_t* K);
int kgwas_kinship_get_stats(const kgwas_kinship* k, double* kernel_ms, uint64_t* launches, uint64_t* rows_fed);
void kgwas_kinship_destroy(kgwas_kinship* k);
/* The whole table over several devices (one process, one thread + session per device, contiguous row shards, integer
 * partials added): hamming [S_f x S_f] and n_used as kgwas_kinship_partials gives them for a single device. */
int kgwas_kinship_table_multi(const int32_t* devices, uint32_t n_devices, kgwas_table* t, uint64_t min_count, uint64_t* hamming,
                              uint64_t* n_used);
/* The matrix text emma_kinship_kmers prints to stdout (:95-111). Returns needed bytes. */
uint64_t kgwas_kinship_format(uint64_t n_acc_file, const uint64_t* K, uint64_t n_used, char* out, uint64_t cap);

/* ------------------------------------------------------------------------------------
 * Pass 2 of associate_kmers (src/associate_kmers.cpp:150-205): <base>.bed/.bim/.fam for one
 * phenotype column from its heap (pop order) — write_PA (src/kmers_multiple_databases.cpp:218-252),
 * BedBimFilesHandle (src/kmer_general.h:133-147), write_fam_file (src/kmer_general.cpp:207-225).
 * The winners' rows are fetched by file row index instead of re-scanning the table.
 * ---------------------------------------------------------------------------------- */
int kgwas_write_plink(const char* out_base, kgwas_table* t, const uint64_t* col, uint64_t n_acc,
                      const char* const* acc_names, const float* y, uint64_t n, const uint64_t* kmer_pop,
                      const uint64_t* row_pop);
/* The same for ALL phenotype columns of a run in one call - what the loop of src/associate_kmers.cpp:167-195 writes from
 * its second pass over the table: column j's files <out_bases[j]>.bed/.bim/.fam from its heap in pop order (n_win[j]
 * entries kmer_pop[j][i], row_pop[j][i]) and its values Y[j * n_acc ..]. The union of the winners' rows is read once
 * (sorted, neighbouring rows in one read, read-ahead requested when the file turns out to be cold), expanded once
 * (word-wise) and written by `threads` host threads (0: the CPUs this process may use). Files are byte-identical to
 * kgwas_write_plink's, which is this call with one column. */
int kgwas_write_plink_many(uint64_t n_cols, const char* const* out_bases, kgwas_table* t, const uint64_t* col, uint64_t n_acc,
                           const char* const* acc_names, const float* Y, const uint64_t* n_win, const uint64_t* const* kmer_pop,
                           const uint64_t* const* row_pop, uint32_t threads);

/* ------------------------------------------------------------------------------------
 * kmers_table_to_bed (src/kmers_table_to_bed.cpp:93-129): the whole table, MAC-filtered on the phenotyped
 * accessions col[0..n_acc), as PLINK files <out_base>.<i>.bed/.bim/.fam, a new file set after every batch_size KEPT
 * k-mers (load_kmers, src/kmers_multiple_databases.cpp:110-113); with unique_patterns only the first k-mer of each
 * presence/absence hash (hash_presence_absence_pattern, :367-375) over all batches
 * (output_plink_bed_file_unique_presence_absence_patterns, :254-264). Per-row work (squeeze, popcount, hash, PLINK
 * bytes) runs on `device`. n_batches / n_written (k-mers written) may be NULL.
 * ---------------------------------------------------------------------------------- */
int kgwas_table_to_bed(kgwas_table* t, const uint64_t* col, uint64_t n_acc, const char* const* acc_names, const float* y,
                       uint64_t min_count, uint64_t batch_size, int unique_patterns, const char* out_base, int device,
                       uint64_t* n_batches, uint64_t* n_written);

/* ------------------------------------------------------------------------------------
 * filter_kmers (src/filter_kmers.cpp): the presence/absence rows of listed k-mers.
 * kgwas_kmer_encode: kmer2bits (src/kmer_general.cpp:260-283) of word[0, len), 1 <= len <= 32 - the canonical code
 * min(b, reverse complement of b); a character other than A, C, G, T -> KGWAS_ERR_FORMAT "Ilegal kmer".
 * kgwas_filter_kmers: the reference's merge-join (:152-177) of the sorted codes (any order; the library sorts a copy,
 * duplicates kept) with the table's rows in file order, exact also where the table's keys descend. Emitted rows go to
 * file_rows[i] (file row index) and rows[i * (1 + W_f) ..] (the raw row), in file order; the caller gives room for
 * min(n, table rows) of them, and either may be NULL. kgwas_filter_kmers_write writes the reference's output file instead
 * (header "kmer\t<name>...", then bits2kmer31(key, k) and "\t0" / "\t1" per accession for each emitted row; k of the table,
 * 1..32), formatted on the device; a failed write (a full disk) is KGWAS_ERR_IO. Both run on `device`.
 * ---------------------------------------------------------------------------------- */
int kgwas_kmer_encode(const char* word, uint64_t len, uint64_t* code);
int kgwas_filter_kmers(kgwas_table* t, const uint64_t* codes, uint64_t n, int32_t device, uint64_t* file_rows, uint64_t* rows,
                       uint64_t* n_found);
int kgwas_filter_kmers_write(kgwas_table* t, const uint64_t* codes, uint64_t n, int32_t device, const char* out_path,
                             uint64_t* n_found);

/* ------------------------------------------------------------------------------------
 * build_kmers_table (src/build_kmers_table.cpp, src/kmers_merge_multiple_databaes.cpp): the k-mers table from the sorted
 * all-k-mers file and the n accessions' sorted k-mer files (64-bit little-endian words, top two bits flags; length size >> 3).
 * Writes <out_base>.table (prefix, n, kmer_len, then one row per used all-k-mers word: the masked word and ceil(n / 64) words
 * of bits) and, when names is not NULL, <out_base>.names (one name per line) before any input is opened. The rows and bits are
 * the reference's, its 5001 key windows and first-insert-wins hash map included, also for inputs that descend or repeat keys
 * (DESIGN.md 4.9); the match runs on `device`. The all-k-mers file is opened first, then the accessions' in order, and the
 * .table is created after all of them: a file of fewer than 8 bytes -> KGWAS_ERR_FORMAT "sorted kmer file is empty: <path>", one
 * that cannot be opened -> KGWAS_ERR_FORMAT "can't open file: <path>". kmer_len must be within 1..31. *n_rows (may be NULL):
 * rows written. Files are opened as they are read, a few at a time: n is not bound by the descriptor limit.
 * ---------------------------------------------------------------------------------- */
int kgwas_build_table(const char* all_kmers_path, const char* const* kmer_paths, const char* const* names, uint64_t n,
                      uint32_t kmer_len, int32_t device, const char* out_base, uint64_t* n_rows);

/* ------------------------------------------------------------------------------------
 * list_kmers_found_in_multiple_samples (src/list_kmers_found_in_multiple_samples.cpp): the k-mers shared by the n accessions'
 * sorted k-mer files (64-bit little-endian words, length size >> 3; bits 62-63 a strand flag: 1 canonical form only, 2
 * non-canonical only, 3 both; bits 0-61 the key). Per key window of the reference (5001 of them) and key it counts the words,
 * count_all, and those with flag 1 and flag 2; a key with count_all >= mac passes when both strand sides, count_canonical +
 * count_both and count_non_canonical + count_both, are >= ceil(min_strand_percent * count_all) as doubles (any double; NaN passes
 * nothing). Writes <out_path> (the passing keys, 8 bytes each, ascending within a window, windows in order), <out_path>
 * .no_pass_kmers (a header, then "k-mer\tall\tcanonical\tnon-canonical\tboth" per key that reached mac and failed),
 * .shareness, .stats.only_canonical, .stats.only_non_canonical and .stats.both ((n + 1) x (n + 1) counts over all distinct
 * keys). counts (may be NULL): keys passed, keys that reached mac but failed the strand rule, keys below mac. The counts are
 * the reference's also for inputs that descend or repeat keys; the counting runs on `device`. The files are
 * opened in order and the outputs created after all of them: a file of fewer than 8 bytes -> KGWAS_ERR_FORMAT "sorted kmer
 * file is empty: <path>", one that cannot be opened -> KGWAS_ERR_FORMAT "can't open file: <path>". Three inputs on which the
 * reference has undefined behaviour are KGWAS_ERR_FORMAT too: n >= 2^20 (refused before any file or the device is touched), a
 * used word with flag 0 (the message names the file), a key counted more than n times in one window (it names the k-mer).
 * kmer_len must be within 1..31. Files are opened as they are read, a few at a time: n is not bound by the descriptor limit.
 * ---------------------------------------------------------------------------------- */
int kgwas_list_kmers(const char* const* kmer_paths, uint64_t n, uint32_t kmer_len, uint64_t mac, double min_strand_percent,
                     int32_t device, const char* out_path, uint64_t counts[3]);

/* ------------------------------------------------------------------------------------
 * count_kmers_with_strand: an accession's sorted k-mer file from its reads. A tool of this project, not a drop-in: it stands
 * where the reference pipeline runs `kmc -ci<T>`, `kmc -ci0 -b` and kmers_add_strand_information (src/
 * kmers_add_strand_information.cpp:32-38,119-145; a KMC database reader, not built here), and its output format, flag rule,
 * sort order and summary numbers are that tool's. The rules:
 * A window is kmer_len consecutive bytes of one read, all of them A, C, G, T in either case; a window with any other byte is
 * skipped, and no window spans two reads or files. Its code a is kgwas_kmer_encode's (A=0, C=1, G=2, T=3, first base most
 * significant), b the code of its reverse complement. If a < b the window's key is a and its flag 0x4000000000000000 (seen in
 * canonical form), otherwise the key is b and the flag 0x8000000000000000 (a palindrome, a == b, gets this one, as
 * is_canonized_kmer_representation_flag gives it). count(key) is the number of windows with that key over all reads, flags(key)
 * the OR of their flags. A key is kept iff ci <= count <= cx. <out_path> holds key | flags of the kept keys, 8 bytes
 * little-endian, ascending by key; a run that keeps nothing writes an empty file. counts (may be NULL): [0] kept keys, [1]
 * distinct oriented k-mers (distinct a), [2] distinct oriented k-mers whose key is kept, [3..6] kept keys with flag 0, 1, 2, 3
 * ([3] is always 0), [7] all counted windows. These are what the three reference commands give for the same reads if KMC
 * counts by these rules: by construction, not checked against a KMC run.
 * kgwas_count_kmers_files: n FASTA or FASTQ files, plain text, "-" standard input; the format is decided per file from its first
 * byte, '>' FASTA, '@' FASTQ, an empty file has no reads, anything else -> KGWAS_ERR_FORMAT "<path>: neither FASTA nor FASTQ".
 * FASTQ is four lines per record ('@...', sequence, '+...', quality - which may begin with '@'); a last record with fewer than
 * four lines, or a record without '@' / '+' at the head of its first / third line, -> KGWAS_ERR_FORMAT naming the file. In
 * FASTA a read is the concatenation of the lines up to the next line that begins with '>'. A trailing '\r' is dropped from
 * every line; a missing final newline is fine. A file that cannot be opened -> KGWAS_ERR_IO "can't open file: <path>".
 * kgwas_count_kmers_bases: the reads as one byte stream in which every byte other than A, C, G, T (either case) separates
 * reads; host memory, or device memory of `device` when on_device is not 0.
 * Both: kmer_len within 1..31, ci > cx -> KGWAS_ERR_ARG, no HIP device -> KGWAS_ERR_DEVICE. All inputs are opened and their
 * format byte checked before <out_path> is created. The bases stay resident on the device and are counted in key-range passes;
 * an input whose bases do not fit beside one pass's buffers -> KGWAS_ERR_ARG with both sizes.
 * ---------------------------------------------------------------------------------- */
int kgwas_count_kmers_files(const char* const* paths, uint64_t n, uint32_t kmer_len, uint64_t ci, uint64_t cx, int32_t device,
                            const char* out_path, uint64_t counts[8]);
int kgwas_count_kmers_bases(const void* bases, uint64_t n_bytes, int on_device, uint32_t kmer_len, uint64_t ci, uint64_t cx,
                            int32_t device, const char* out_path, uint64_t counts[8]);

/* ------------------------------------------------------------------------------------
 * SNP twin of the scorer: MultipleSNPsDataBases (src/snps_multiple_databases.h:25-63) for associate_snps
 * (src/associate_snps.cpp). open: <base>.fam/.bed with the phenotyped samples in phenotype order (ctor, :66-146,
 * error texts included); scores: calculate_grammmar_approx_association (:155-172) of every SNP for every column of
 * Y[n_pheno][n_samples], scores[j*n_snps + i], on `device`; best: get_most_associated_snps (:229-241) per column -
 * counts[j] sorted SNP indices at indices[j*topn ...]; write: output_plink_bed_file (:252-286) - list l
 * (counts[l] sorted indices at indices[l*stride ...]) to out_bases[l].bed/.bim.
 * ---------------------------------------------------------------------------------- */
typedef struct kgwas_snps kgwas_snps;
int kgwas_snps_open(const char* base_bedbim, const char* const* samples, uint64_t n_samples, kgwas_snps** out);
int kgwas_snps_info(const kgwas_snps* s, uint64_t* n_snps, uint64_t* n_samples_file, uint64_t* bytes_per_snp);
int kgwas_snps_scores(kgwas_snps* s, const float* Y, uint64_t n_pheno, double mac, int device, double* scores);
int kgwas_snps_best(kgwas_snps* s, const float* Y, uint64_t n_pheno, uint64_t topn, double mac, int device, uint64_t* counts,
                    uint64_t* indices);
int kgwas_snps_write(kgwas_snps* s, uint64_t n_lists, const char* const* out_bases, const uint64_t* counts,
                     const uint64_t* indices, uint64_t stride);
void kgwas_snps_close(kgwas_snps* s);

/* ------------------------------------------------------------------------------------
 * SNP kinship = emma_kinship (src/emma_kinship.cpp): the EMMA kinship of a PLINK SNP matrix. For every SNP with at least
 * one called sample and every pair r > c, K[r][c] += a_r*a_c + (1-a_r)*(1-a_c), once with pass A's values (hom 0, het 0,
 * hom-alt 1, missing n_alt/n_total) and once with pass B's (het 1, missing (n_alt+n_het)/n_total); each pair's sum is
 * accumulated in SNP order with one IEEE rounding per operation, so it is bit-identical to the reference's.
 * open     : <base>.bed / <base>.fam guards with the reference's messages in its order ("error:\t" + text; missing files
 *            KGWAS_ERR_IO, sizes KGWAS_ERR_FORMAT; a .fam without lines KGWAS_ERR_ARG - the reference divides by zero),
 *            all before the device is touched; then the session on `device`
 * info     : S samples (lines of the .fam), M SNPs, bytes per SNP
 * feed_bed : n_snps SNPs of the .bed body (file layout, without the 3 magic bytes) from host memory, after those fed
 *            before (several feeds equal one)
 * feed_file: the whole .bed body, streamed in chunks (file read, copy and kernels overlap)
 * sums     : the undivided sums, lower[r * S + c] for c < r (the other entries 0), and the SNPs used so far
 * matrix   : the finished S x S matrix: sums / (2 n_used) mirrored, diagonal 1 (0 / 0 = -nan when no SNP was used)
 * format   : the text emma_kinship prints for K (plot_kinship, :55-68). Returns needed bytes.
 * ---------------------------------------------------------------------------------- */
typedef struct kgwas_snpkin kgwas_snpkin;
int kgwas_snpkin_open(const char* base_bedbim, int32_t device, kgwas_snpkin** out);
int kgwas_snpkin_info(const kgwas_snpkin* h, uint64_t* n_samples, uint64_t* n_snps, uint64_t* bytes_per_snp);
int kgwas_snpkin_feed_bed(kgwas_snpkin* h, const uint8_t* body, uint64_t n_snps);
int kgwas_snpkin_feed_file(kgwas_snpkin* h);
int kgwas_snpkin_sums(kgwas_snpkin* h, double* lower, uint64_t* n_used);
int kgwas_snpkin_matrix(kgwas_snpkin* h, double* K, uint64_t* n_used);
uint64_t kgwas_snpkin_format(uint64_t n_samples, const double* K, char* out, uint64_t cap);
void kgwas_snpkin_close(kgwas_snpkin* h);

/* ------------------------------------------------------------------------------------
 * lmm_lrt: the mixed-model likelihood-ratio test of the best k-mers (or SNPs). A tool of this project, not a drop-in: it
 * stands where the pipeline starts `gemma -bfile B -lmm 2 -k pheno.kinship -outdir D -o NAME -maf f -miss 0.5` once per
 * phenotype column (kmers_gwas.py:150-165) and reads the p_lrt column of the results (functions.py:93-112). The statistic is
 * the ML likelihood-ratio test of y = W a + x b + u + e, u ~ N(0, lambda K / tau), e ~ N(0, I / tau), W = 1; the reference tree
 * ships an independent formulation of it in src/R/emma.R:495-616 (emma.ML.LRT, emma.MLE, emma.eigen.R.wo.Z,
 * emma.delta.ML.LL.wo.Z), which the tests restate. DESIGN.md 4.12 has the formulas and the fixed maximisation procedure.
 * Added in ABI version 13.
 * sym_eigen: K (n x n, row-major; its symmetric part is used) = U diag(d) U^T, d ascending, U row-major with eigenvector c in
 *            column c. Householder tridiagonalisation and implicit QL on `threads` host threads (0: the CPUs this process may
 *            use); the result does not depend on `threads`. Needs no GPU.
 * create   : eigendecomposes K, sets |d_i| < 1e-8 to 0 and refuses a d_i < -1e-8 with KGWAS_ERR_FORMAT "Kinship matrix is not
 *            positive semi-definite" (transform_and_permute_phenotypes.R:54), all before the device is touched; then the session
 *            on `device`. lambda is searched in [lmin, lmax] (GEMMA's defaults: 1e-5, 1e5). chunk_variants (0: 10240, rounded up
 *            to 32) variants are on the device at a time. n within 3..65535.
 * null     : the null model's maximised log-likelihood and its lambda for phenotype y[n] (finite, not constant).
 * test_bed : n_variants variants of a SNP-major .bed body (file layout without the 3 magic bytes, (n + 3) / 4 bytes each, the
 *            handle's individuals in order). Code 00 -> 2, 10 -> 1, 11 -> 0, 01 (missing) -> the mean of the others; af = mean /
 *            2, n_miss = number of 01 codes. A variant is not tested when min(af, 1 - af) < maf, when n_miss / n > miss or when
 *            it is constant: tested = 0 and lrt, lambda, p are NaN. Otherwise lrt = max(0, 2 (l1 - l0)), lambda the H1 maximiser
 *            and p = erfc(sqrt(lrt / 2)). Outputs are host arrays of n_variants entries; any may be NULL. A variant's numbers
 *            are bit-identical from run to run, in any order and for any chunk_variants.
 * run_files: the lmm_lrt tool's file layer. kinship_path: a text matrix, one row per .fam line (a different number of rows or
 *            columns -> KGWAS_ERR_FORMAT); per bed i, <bfile_bases[i]>.bed/.bim/.fam in and out_paths[i] out (chr rs ps n_miss
 *            allele1 allele0 af l_mle p_lrt, tab-separated, tested variants in .bim order) plus a log beside it (".assoc.txt"
 *            replaced by ".log.txt"). The phenotype is field 5 + pheno_col of the .fam; individuals with "-9" or "NA" are
 *            dropped from K, y and the .bed. Consecutive beds that keep the same individuals share one eigendecomposition.
 *            total (may be NULL): the run's summed stats.
 * test_bed_multi (ABI version 14): n_pheno phenotype columns Y[n_pheno][n] against ONE .bed body, the shape of the pipeline's
 *            SNP branch (kmers_gwas.py:193-223: the phenotype and its permutations over one SNP panel). The .bed is copied, decoded
 *            and rotated once per chunk, and the grid sums without y are made once; only the sums with y and the refinement run
 *            per column. lrt, lambda, p are [n_pheno][n_variants]; logl0, lambda0 [n_pheno]; af, n_miss, tested [n_variants]; any
 *            may be NULL. Every value has the bits that kgwas_lmm_null / kgwas_lmm_test_bed give for that column alone, for any
 *            chunk_variants and any order of the columns. n_pheno == 0, a non-finite value or a constant column -> KGWAS_ERR_ARG
 *            (the message names the column, from 0) before any device work; the handle stays usable. The call leaves the
 *            phenotype that kgwas_lmm_null / kgwas_lmm_test_bed cache untouched. Its device buffers are allocated at the first
 *            such call (0.55 GB at the default chunk_variants). Stats: variants_read counts a variant once, variants_tested once
 *            per column; grid_ms takes the shared and the per-column sums.
 * run_file_multi (ABI version 14): run_files for ONE bfile and n_cols columns of its .fam (pheno_cols, from 1): the .fam, the
 *            .bim, the .bed and the kinship matrix are read once, K is eigendecomposed once, and out_paths[k] (with its log) gets
 *            what run_files writes for column pheno_cols[k]. All columns must mark the same .fam lines as missing; otherwise
 *            KGWAS_ERR_FORMAT, naming the first column that differs from the first one.
 * test_table (ABI version 15): the exact test of EVERY k-mer of a k-mers table, without a .bed in between, and the best best_n of
 *            them. col[n_acc] maps the handle's individuals, in order, to table columns (kgwas_table_column_map); n_acc must be the
 *            handle's n. A row is tested iff kgwas_table_to_bed would write it at this min_count (n_acc >= min_count, presence
 *            count n1 >= min_count, n1 <= n_acc - min_count) AND test_bed would test its .bed row at this maf (not constant,
 *            min(af, 1 - af) >= maf with af = (n_acc - n1) / n_acc computed as test_bed does; a table has no missing calls). The
 *            device squeezes, counts, flags and compacts a piece of rows; only tested rows are rotated. Their lrt, lambda, p and af
 *            have the bits that kgwas_table_to_bed followed by kgwas_lmm_test_bed gives. Kept are the best_n tested rows with the
 *            largest lrt, ties to the smaller table row - the same set for any piece size and chunk_variants. Outputs are host
 *            arrays of best_n entries in table row order (row: the table row index, kmer: its 2-bit word), *n_kept <= best_n of
 *            them valid; any output may be NULL. best_n == 0, a NULL h, y, t or col, n_acc != n or a column index out of range
 *            -> KGWAS_ERR_ARG. The table file is read on a host thread while the device works on the piece before. Stats:
 *            variants_read counts table rows, variants_tested tested rows; rotate_ms takes the front end too. KGWAS_LMM_PIECE_ROWS
 *            (test hook) sets the rows per piece.
 * run_table (ABI version 15): the file layer of lmm_lrt --kmers_table. Accessions and their order are the phenotype file's
 *            (kgwas_pheno_load; every one must be a table column), the kinship text has one row per accession, y is column
 *            pheno_col (from 1) of the phenotype file: the loader's float, written as kgwas_table_to_bed writes it into a .fam
 *            (ostream's default format) and parsed as read_fam parses a .fam field, so both routes see the same doubles. A value
 *            that prints as "-9" or "NA" (missing in a .fam) is refused with KGWAS_ERR_FORMAT. min_count = kgwas_min_count(n, maf,
 *            mac). out_path gets the header and one line per kept k-mer in table order (chr 0, rs the k-mer, ps 0, n_miss 0,
 *            allele1 0, allele0 1, af, l_mle, p_lrt: the bytes run_files writes for that k-mer of kgwas_table_to_bed's files),
 *            the log beside it adds rows_read, rows_tested, rows_kept and best_n.
 * test_table_multi (ABI version 15): test_table for n_pheno columns Y[n_pheno][n] in ONE pass over the table - the phenotype and
 *            its permutations, whose best p-values give the pipeline its threshold (kmers_gwas.py:245-253). A piece is read,
 *            squeezed, flagged, compacted and rotated once; the grid sums without y run once per sub-chunk; the sums with y, the
 *            refinement and a select kernel run per block of 32 columns. The select kernel hands the host only the (column, row)
 *            pairs that can still enter the column's best best_n: all while the column's heap is not full, then those whose lrt
 *            is larger than the lrt of the heap's worst hit as the host knew it before the launch (rows arrive in increasing order,
 *            so a later row with an equal lrt ranks after the kept one). The host heaps still decide. row, kmer, lrt, lambda, p,
 *            af are [n_pheno][best_n] (column k's entries start at k best_n, in table row order, n_kept[k] of them valid); n_kept,
 *            logl0, lambda0 [n_pheno]; any output may be NULL. Column k's kept rows and numbers have the bits kgwas_lmm_test_table
 *            gives for Y[k] alone, and logl0 / lambda0 those of kgwas_lmm_null, for any piece size, chunk_variants and order of the
 *            columns. *pairs_shipped: the records the device handed to the host, at most rows_tested x n_pheno. Errors as
 *            test_table, and n_pheno == 0, a non-finite value or a constant column -> KGWAS_ERR_ARG (the message names the column,
 *            from 0), all before any device work; the handle stays usable and the phenotype cached by kgwas_lmm_null stays
 *            untouched. Stats: variants_read counts table rows, variants_tested a tested row once per column; rotate_ms takes the
 *            front end and the rotation, grid_ms the shared and the per-column sums, refine_ms the refinement and the select
 *            kernel. The selection's buffers (32 chunk_variants records of 56 bytes on the device and pinned on the host) are
 *            allocated at the first such call. KGWAS_LMM_TABLE_SELECT=0 (test hook) lets every pair through; the results are the same.
 * run_table_multi (ABI version 15): run_table for n_cols columns of the phenotype file (pheno_cols, from 1) in one pass: the
 *            phenotype file, the table and the kinship text are read once, K is eigendecomposed once, and out_paths[k] with its
 *            log gets what run_table writes for column pheno_cols[k] (the kernels' times in the logs are the shared pass's).
 * read_kinship / read_fam / format_assoc: the parsers and the line formatter of run_files (no GPU). read_fam gives every line's
 *            value (NaN when missing) and keep flag, up to cap entries, and the number of lines. format_assoc returns the bytes
 *            needed and writes them if cap allows; chr == NULL gives the header line.
 *
 * -lmm 4 (after ABI version 15, no bump: probe by symbol). Beside the LRT: the REML effect estimate with its standard error, the
 * Wald test and the score test - the forms GEMMA documents for -lmm 1 / 3 / 4, not checked against a GEMMA run. With the rotated,
 * centred vectors, h_i = 1 / (lambda d_i + 1), the h-weighted sums ww .. xy and a.w the Schur complement after w:
 *     lR(lambda) = df/2 (log(df / 2 pi) - 1) + 1/2 sum log h_i - 1/2 (log ww + log xx.w) - df/2 log RSS1,  df = n - 2,
 * l_remle its maximiser over [lmin, lmax] by the procedure that finds l_mle (a boundary optimum is lmin or lmax exactly);
 *     beta = xy.w / xx.w, se = sqrt(RSS1 / (df xx.w)), F_wald = (yy.w - RSS1) df / RSS1 = (beta / se)^2 at l_remle,
 *     F_score = n xy.w^2 / (xx.w yy.w) at lambda0, the null model's ML lambda (kgwas_lmm_null),
 * p_wald and p_score their F(1, df) tails. beta is per unit of the decoded dosage (code 00 -> 2): the allele that af counts.
 * null_reml: the null model by REML, lR0(lambda) = df0/2 (log(df0 / 2 pi) - 1) + 1/2 sum log h - 1/2 log ww - df0/2 log yy.w with
 *            df0 = n - 1, the same maximisation; ve = yy.w / df0 and vg = lambda ve at the maximiser (emma.REMLE's ve and vg, delta =
 *            1 / lambda). Any output may be NULL. The phenotype is cached as kgwas_lmm_null caches it.
 * test_bed_all: test_bed with five more outputs (any may be NULL). An untested variant has NaN in all eight statistics. lrt,
 *            lambda_mle, p_lrt, af, n_miss and tested have the bits of kgwas_lmm_test_bed, and all eight are bit-identical from run
 *            to run, in any variant order and for any chunk_variants.
 * run_files_all: run_files writing the -lmm 4 file: chr rs ps n_miss allele1 allele0 af beta se l_remle l_mle p_wald p_lrt p_score
 *            (columns 1-7, l_mle and p_lrt with the bytes of the -lmm 2 file); the log has the -lmm 2 log's lines under its own
 *            title and, behind logl_H0, lambda0_remle, logl_remle_H0, vg and ve.
 * format_assoc4: format_assoc for that file; af as %.3f, the seven numbers as %.6e (a p below the normal doubles prints as a
 *            subnormal or 0, which parses back).
 * fdist_tail: Q(F; 1, df) = I_x(df / 2, 1 / 2), x = df / (df + F): the tail both tests use, the host instance of the function the
 *            kernel calls (no GPU). F <= 0 -> 1; relative error below 1e-9 for df <= 65533 also where p is tiny.
 *
 * Covariates (after ABI version 15, no bump: probe by symbol). The model y = W a + x b + u + e with W (n x q, 1 <= q <= 8) in place
 * of W = 1. The column space of W must hold the constant vector (give W a column of 1s). Every n - 1 above becomes n - q and every
 * n - 2 becomes n - q - 1: the REML df, ve = RSS0 / (n - q), the F(1, n - q - 1) tails. n >= q + 2.
 * set_covariates: W[n][q] row-major for every later kgwas_lmm_null, _null_reml, _test_bed, _test_bed_all and _test_table on the
 *            handle; q = 0 restores W = 1 and the bits of a handle that never had covariates. W is replaced by an orthonormal
 *            basis of its columns (modified Gram-Schmidt, in column order), so every output but logl0_reml is the same for W and
 *            W A, A invertible, to rounding; logl0_reml is the restricted likelihood of W as given. Refused (KGWAS_ERR_ARG, nothing
 *            changed): q > 8, a value that is not finite, n < q + 2, a column whose remainder after the columns before it is
 *            <= 1e-8 of its norm (rank), a constant vector whose remainder is > 1e-8 sqrt(n) (span). The cached null models are
 *            forgotten. A variant that lies in the span of W to rounding has no test and is not detected. The multi-phenotype
 *            passes (kgwas_lmm_test_bed_multi, kgwas_lmm_test_table_multi) refuse a handle with covariates.
 * read_covariates: GEMMA's -c file (no GPU): one row per individual, whitespace-separated numbers, NA for a missing value, every
 *            row with the same number of fields. *q_out = q always. values[row][q] (NaN where NA) and keep[row] (0 where the row
 *            has an NA; one byte per row) are written when rows * q <= cap, cap counting the doubles of `values`; otherwise
 *            neither is touched. The call does not return the number of rows: pass it as n_expected (a file with another number
 *            is refused) and size both arrays by it; n_expected == 0 accepts any number and is of use only to learn q. Lines
 *            that are empty or hold only blanks are skipped and do not count as rows, as in the kinship and .fam parsers, so a
 *            stray blank line shifts nothing but a lost row does: the row count against n_expected is the check for that.
 * run_files_cov: run_files (all_tests = 0) or run_files_all (all_tests != 0) with covar_path, rows in .fam order: an individual is
 *            used iff its phenotype is present and no covariate is NA. The log gains the lines covariates and n_covariates behind
 *            kinship. covar_path == NULL: exactly run_files / run_files_all.
 * run_table_cov: run_table with covar_path, one row per accession of the phenotype file in its order; NA is refused.
 *
 * The pattern cache (after ABI version 15, no bump: probe by symbol). Rows of a k-mers table repeat presence/absence patterns, and
 * two rows with the same pattern over the handle's individuals have the same lrt, lambda, p and af, bit for bit.
 * test_table_unique: test_table (with or without covariates on the handle) in which each distinct tested pattern goes through
 *            rotate, grid and refine once and every other row with it takes the stored result. A cache and nothing more: row, kmer,
 *            lrt, lambda, p, af, *n_kept, *rows_read and *rows_tested are kgwas_lmm_test_table's, byte for byte, for any
 *            max_patterns, piece size and chunk_variants, also when tags collide or the cache is full. The cache is a hash table
 *            on the device with max_patterns slots, rounded down to a power of two (at most 2^30), of 40 bytes + the code row
 *            (n rounded up to 16, / 4 bytes) each; it is allocated for the call and empty at its start (results depend on y and
 *            the covariates). A tested row hashes its code row to a 64-bit tag and looks at up to 16 slots in a row. *u (may be
 *            NULL): slots; patterns_cached, the rows that took a new slot; rows_from_cache, the rows whose code row equalled
 *            their slot's (not rotated); rows_collided, the rows whose slot held another code row with their tag; rows_rejected,
 *            the rows that found no slot; rows_rotated. rows_tested = patterns_cached + rows_from_cache + rows_collided +
 *            rows_rejected, rows_rotated = rows_tested - rows_from_cache. With nothing rejected the counters are the same in
 *            every run and patterns_cached + rows_collided is at least the number of distinct tested patterns (equal to it, and
 *            rows_collided 0, unless two patterns share a 64-bit tag). max_patterns < 64 -> KGWAS_ERR_ARG before any device
 *            work, *u and the handle's stats untouched, the handle still usable; the other errors are test_table's. Stats as
 *            test_table (variants_tested counts tested rows); rotate_ms takes the cache's kernels too.
 *            KGWAS_LMM_PATTERN_TAG_BITS=k (test hook) cuts the tags to k bits, so that they collide; the results are the same.
 * run_table_unique: run_table_cov (covar_path may be NULL: run_table) through test_table_unique with a cache of cache_mib MiB: as
 *            many slots as fit, rounded down to a power of two. out_path gets the bytes of the run without the cache; the log gains,
 *            behind its present lines, pattern_cache_slots, patterns_cached, rows_from_cache, rows_collided, rows_rejected and
 *            rows_rotated. cache_mib == 0, or fewer than 64 slots -> KGWAS_ERR_ARG.
 *
 * The dead-pattern skip (after ABI version 15, no bump: probe by symbol). In the multi-phenotype table pass a tested row whose
 * (column, row) pairs were all computed and of which the select kernel shipped none met only full heaps and lay at or below every
 * column's threshold. A full heap stays full, its worst lrt never falls, and a later row with the same pattern has the same lrt in
 * every column, bit for bit: it would ship nothing either. Such a pattern is dead.
 * test_table_multi_skip: test_table_multi that remembers the tested patterns in a hash table on the device (the pattern cache's:
 *            max_patterns slots rounded down to a power of two, at most 2^30, 16 tries per row, tags of 64 bits) with one state
 *            word per slot and no results: 16 bytes + the code row (n rounded up to 16, / 4 bytes) each, allocated for the call
 *            and empty at its start (what ships depends on Y). A row whose pattern was dead when its piece of rows began is left
 *            out of the rotation, the grid sums, the refinement and the selection; every other tested row is computed, in row
 *            order, and marks its pattern dead if it shipped no pair. Every output of test_table_multi, *pairs_shipped included,
 *            is test_table_multi's byte for byte, for any max_patterns, piece size and chunk_variants, also when tags collide or
 *            the table is full. *u (may be NULL): slots; patterns_cached, the rows that took a new slot; patterns_dead, the slots
 *            dead at the end; rows_skipped; rows_collided and rows_rejected (computed, and they never mark a pattern); rows_rotated,
 *            the rows computed. *rows_tested = rows_rotated + rows_skipped counts rows, not rows x columns. With nothing rejected
 *            the counters are the same in every run. While a column's heap is open (fewer than best_n tested rows so far, or
 *            KGWAS_LMM_TABLE_SELECT=0) nothing dies and nothing is skipped. max_patterns < 64 -> KGWAS_ERR_ARG before any device
 *            work, *u and the handle's stats untouched; a handle with covariates is refused as by test_table_multi; the other
 *            errors are test_table_multi's. Stats as test_table_multi (variants_tested counts a tested row once per column,
 *            skipped or not); rotate_ms takes the table's kernels. KGWAS_LMM_PATTERN_TAG_BITS as for test_table_unique.
 * run_table_multi_skip: run_table_multi through test_table_multi_skip with a table of cache_mib MiB: as many slots as fit, rounded
 *            down to a power of two. The files get the bytes of run_table_multi; every log gains, behind its present lines,
 *            pattern_skip_slots, patterns_cached, patterns_dead, rows_skipped, rows_collided, rows_rejected and rows_rotated.
 *            cache_mib == 0, or fewer than 64 slots -> KGWAS_ERR_ARG.
 * ---------------------------------------------------------------------------------- */
typedef struct kgwas_lmm kgwas_lmm;
typedef struct kgwas_lmm_stats {
    double eigen_ms, rotate_ms, grid_ms, refine_ms; /* host eigendecomposition; kernels: prep + rotate, grid sums, refine */
    uint64_t variants_read, variants_tested, chunks, eigendecompositions, n_individuals;
} kgwas_lmm_stats;
int kgwas_sym_eigen(uint64_t n, const double* K, double* d, double* U, uint32_t threads);
int kgwas_lmm_create(uint64_t n, const double* K, int32_t device, double lmin, double lmax, uint64_t chunk_variants, kgwas_lmm** out);
int kgwas_lmm_null(kgwas_lmm* h, const double* y, double* logl0, double* lambda0);
int kgwas_lmm_test_bed(kgwas_lmm* h, const double* y, const uint8_t* bed_body, uint64_t n_variants, double maf, double miss, double* lrt,
                       double* lambda, double* p, double* af, uint32_t* n_miss, uint8_t* tested);
int kgwas_lmm_run_files(const char* kinship_path, uint64_t n_beds, const char* const* bfile_bases, const char* const* out_paths,
                        uint32_t pheno_col, double maf, double miss, double lmin, double lmax, uint64_t chunk_variants, int32_t device,
                        kgwas_lmm_stats* total);
int kgwas_lmm_test_bed_multi(kgwas_lmm* h, uint32_t n_pheno, const double* Y, const uint8_t* bed_body, uint64_t n_variants, double maf,
                             double miss, double* lrt, double* lambda, double* p, double* logl0, double* lambda0, double* af,
                             uint32_t* n_miss, uint8_t* tested);
int kgwas_lmm_run_file_multi(const char* kinship_path, const char* bfile_base, uint32_t n_cols, const uint32_t* pheno_cols,
                             const char* const* out_paths, double maf, double miss, double lmin, double lmax, uint64_t chunk_variants,
                             int32_t device, kgwas_lmm_stats* total);
int kgwas_lmm_test_table(kgwas_lmm* h, const double* y, kgwas_table* t, const uint64_t* col, uint64_t n_acc, uint64_t min_count, double maf,
                         uint64_t best_n, uint64_t* row, uint64_t* kmer, double* lrt, double* lambda, double* p, double* af,
                         uint64_t* n_kept, uint64_t* rows_read, uint64_t* rows_tested);
int kgwas_lmm_run_table(const char* kinship_path, const char* table_base, uint32_t kmer_len, const char* pheno_path, uint32_t pheno_col,
                        uint64_t mac, double maf, uint64_t best_n, double lmin, double lmax, uint64_t chunk_variants, int32_t device,
                        const char* out_path, kgwas_lmm_stats* total);
int kgwas_lmm_test_table_multi(kgwas_lmm* h, uint32_t n_pheno, const double* Y, kgwas_table* t, const uint64_t* col, uint64_t n_acc,
                               uint64_t min_count, double maf, uint64_t best_n, uint64_t* row, uint64_t* kmer, double* lrt, double* lambda,
                               double* p, double* af, uint64_t* n_kept, double* logl0, double* lambda0, uint64_t* rows_read,
                               uint64_t* rows_tested, uint64_t* pairs_shipped);
int kgwas_lmm_run_table_multi(const char* kinship_path, const char* table_base, uint32_t kmer_len, const char* pheno_path, uint32_t n_cols,
                              const uint32_t* pheno_cols, const char* const* out_paths, uint64_t mac, double maf, uint64_t best_n,
                              double lmin, double lmax, uint64_t chunk_variants, int32_t device, kgwas_lmm_stats* total);
int kgwas_lmm_get_stats(const kgwas_lmm* h, kgwas_lmm_stats* out);
void kgwas_lmm_destroy(kgwas_lmm* h);
int kgwas_lmm_read_kinship(const char* path, uint64_t n_expected, double* K);
int kgwas_lmm_read_fam(const char* path, uint32_t pheno_col, uint64_t cap, double* values, uint8_t* keep, uint64_t* n_lines);
uint64_t kgwas_lmm_format_assoc(const char* chr, const char* rs, const char* ps, uint32_t n_miss, const char* allele1, const char* allele0,
                                double af, double l_mle, double p_lrt, char* out, uint64_t cap);
int kgwas_lmm_null_reml(kgwas_lmm* h, const double* y, double* logl0_reml, double* lambda0_reml, double* vg, double* ve);
int kgwas_lmm_test_bed_all(kgwas_lmm* h, const double* y, const uint8_t* bed_body, uint64_t n_variants, double maf, double miss, double* lrt,
                           double* lambda_mle, double* p_lrt, double* beta, double* se, double* lambda_remle, double* p_wald,
                           double* p_score, double* af, uint32_t* n_miss, uint8_t* tested);
int kgwas_lmm_run_files_all(const char* kinship_path, uint64_t n_beds, const char* const* bfile_bases, const char* const* out_paths,
                            uint32_t pheno_col, double maf, double miss, double lmin, double lmax, uint64_t chunk_variants, int32_t device,
                            kgwas_lmm_stats* total);
uint64_t kgwas_lmm_format_assoc4(const char* chr, const char* rs, const char* ps, uint32_t n_miss, const char* allele1, const char* allele0,
                                 double af, double beta, double se, double l_remle, double l_mle, double p_wald, double p_lrt, double p_score,
                                 char* out, uint64_t cap);
double kgwas_fdist_tail(double F, double df);
int kgwas_lmm_set_covariates(kgwas_lmm* h, uint32_t q, const double* W);
int kgwas_lmm_read_covariates(const char* path, uint64_t n_expected, uint64_t cap, double* values, uint8_t* keep, uint32_t* q_out);
int kgwas_lmm_run_files_cov(const char* kinship_path, const char* covar_path, uint64_t n_beds, const char* const* bfile_bases,
                            const char* const* out_paths, uint32_t pheno_col, double maf, double miss, double lmin, double lmax,
                            uint64_t chunk_variants, int32_t device, int32_t all_tests, kgwas_lmm_stats* total);
int kgwas_lmm_run_table_cov(const char* kinship_path, const char* covar_path, const char* table_base, uint32_t kmer_len,
                            const char* pheno_path, uint32_t pheno_col, uint64_t mac, double maf, uint64_t best_n, double lmin, double lmax,
                            uint64_t chunk_variants, int32_t device, const char* out_path, kgwas_lmm_stats* total);
typedef struct kgwas_lmm_unique_stats {
    uint64_t slots, patterns_cached, rows_from_cache, rows_collided, rows_rejected, rows_rotated;
} kgwas_lmm_unique_stats;
int kgwas_lmm_test_table_unique(kgwas_lmm* h, const double* y, kgwas_table* t, const uint64_t* col, uint64_t n_acc, uint64_t min_count,
                                double maf, uint64_t best_n, uint64_t* row, uint64_t* kmer, double* lrt, double* lambda, double* p, double* af,
                                uint64_t* n_kept, uint64_t* rows_read, uint64_t* rows_tested, uint64_t max_patterns,
                                kgwas_lmm_unique_stats* u);
int kgwas_lmm_run_table_unique(const char* kinship_path, const char* covar_path, const char* table_base, uint32_t kmer_len,
                               const char* pheno_path, uint32_t pheno_col, uint64_t mac, double maf, uint64_t best_n, double lmin,
                               double lmax, uint64_t chunk_variants, int32_t device, const char* out_path, kgwas_lmm_stats* total,
                               uint64_t cache_mib, kgwas_lmm_unique_stats* u);
typedef struct kgwas_lmm_skip_stats {
    uint64_t slots, patterns_cached, patterns_dead, rows_skipped, rows_collided, rows_rejected, rows_rotated;
} kgwas_lmm_skip_stats;
int kgwas_lmm_test_table_multi_skip(kgwas_lmm* h, uint32_t n_pheno, const double* Y, kgwas_table* t, const uint64_t* col, uint64_t n_acc,
                                    uint64_t min_count, double maf, uint64_t best_n, uint64_t* row, uint64_t* kmer, double* lrt,
                                    double* lambda, double* p, double* af, uint64_t* n_kept, double* logl0, double* lambda0,
                                    uint64_t* rows_read, uint64_t* rows_tested, uint64_t* pairs_shipped, uint64_t max_patterns,
                                    kgwas_lmm_skip_stats* u);
int kgwas_lmm_run_table_multi_skip(const char* kinship_path, const char* table_base, uint32_t kmer_len, const char* pheno_path,
                                   uint32_t n_cols, const uint32_t* pheno_cols, const char* const* out_paths, uint64_t mac, double maf,
                                   uint64_t best_n, double lmin, double lmax, uint64_t chunk_variants, int32_t device,
                                   kgwas_lmm_stats* total, uint64_t cache_mib, kgwas_lmm_skip_stats* u);

/* ------------------------------------------------------------------------------------
 * clump_kmers: the k-mers of an association file grouped by linkage disequilibrium, the r^2 between two presence/absence
 * patterns - how many independent signals a list of hits holds. A tool of this project's own (the reference stops at the
 * list). For k-mers a, b over the n accessions in use, with presence counts ca, cb and n11 accessions that have both,
 *     num = (n n11 - ca cb)^2,  den = ca (n - ca) cb (n - cb),  r^2 = num / den;
 * the pair is LINKED iff den > 0 and num * 1000000 >= r2_millionths * den, decided in 128-bit integers on the device: no
 * rounding anywhere. A constant row (den = 0) is linked to nothing.
 *
 * kgwas_r2_millionths: the threshold's decimal text ("0.8", "1", ".25") -> integer millionths, read digit by digit, never
 * through a double; KGWAS_ERR_ARG unless it has at most 6 digits after the point and 0 < t <= 1.
 * kgwas_kmers_ld: bits[n_kmers][words_per_row], bit i of a row = accession i (bits at or past n_acc are ignored) ->
 * adj[n_kmers][ceil(n_kmers / 32)], the upper triangle of the link matrix: adj[a][b / 32] bit b % 32 is 1 iff b > a and the
 * pair is linked; the diagonal and the lower triangle are zero. n1[n_kmers] (may be NULL) gets the presence counts. The counts
 * n11 come from the matrix cores (block-scaled FP4 MFMA, float32 accumulation: exact) and never leave the registers. The
 * matrix is produced in blocks of tile_rows consecutive rows a (rounded up to a multiple of 64; 0: the library picks as many as
 * make a block of at most 256 MiB), a block's copy back overlapping the next block's kernel. Checked before any device call
 * (KGWAS_ERR_ARG): null bits or adj, n_acc of 0 or above 8192 (the predicate's integers are sized for that), words_per_row
 * below ceil(n_acc / 64), r2_millionths of 0 or above 1000000, n_kmers above 2^20.
 * kgwas_clump_kmers_run: the tool. assoc_path is an lmm_lrt or GEMMA .assoc.txt: the columns `rs` (the k-mer's letters) and
 * `p_lrt` are found by their names in the header. Refused by name (KGWAS_ERR_FORMAT): an rs of another length than kmer_len or
 * with an illegal letter, a k-mer given twice, a line with too few fields, a p that is not a number - all before the table is
 * opened. The hits with p <= p_max (+inf: all) are taken in p order, ties in file order; their rows come from the table
 * <table_base>.table by kgwas_filter_kmers' search (a hit the table lacks is an error that names it), squeezed to the
 * accessions of pheno_path in its order (NULL: every accession of the table). Clumping: rows are walked in p order, a row no
 * lead has taken becomes a lead and takes every later row linked to it and not yet taken. out_path gets a header and one line
 * per used hit in the file's order: rs, p_lrt (the field's own text), clump (from 1, in lead order), lead (its rs), r2 against
 * the lead (%.6f; 1.000000 for a lead, nan for a constant row, which is a lead alone), n1, n11 (accessions shared with the
 * lead); out_path + ".log.txt" the inputs and the counters. *st (may be NULL) is written when the call succeeds.
 * ---------------------------------------------------------------------------------- */
typedef struct kgwas_clump_stats {
    uint64_t hits_read, hits_used, clumps, largest_clump, linked_pairs, accessions;
    double search_ms, ld_ms, clump_ms; /* the table search, the LD kernels (events around them), the host's clump pass */
} kgwas_clump_stats;
int kgwas_r2_millionths(const char* text, uint32_t* r2_millionths);
int kgwas_kmers_ld(const uint64_t* bits, uint64_t n_kmers, uint64_t words_per_row, uint64_t n_acc, uint32_t r2_millionths, int32_t device,
                   uint64_t tile_rows, uint32_t* adj, uint32_t* n1);
int kgwas_clump_kmers_run(const char* table_base, uint32_t kmer_len, const char* pheno_path, const char* assoc_path, uint32_t r2_millionths,
                          double p_max, int32_t device, uint64_t tile_rows, const char* out_path, kgwas_clump_stats* st);

/* ------------------------------------------------------------------------------------
 * proxy_kmers: every k-mer of the table in LD with a lead k-mer - the step after clump_kmers, which ends with one lead per
 * signal: the k-mers that travel with a lead are the ones to assemble (fetch_reads, below) or map (locate_kmers, below). A tool of this project's own. A row of the table
 * is a PROXY of a lead iff the pair is linked by clump_kmers' predicate (above: num * 1000000 >= r2_millionths * den, den > 0,
 * in 128-bit integers on the device). Every (lead, row) pair is tested, the lead's own row included: a non-constant lead finds
 * itself, a constant lead finds nothing, a complement is a proxy (phase -).
 *
 * kgwas_kmers_ld_proxies: the array level. lead_bits[n_leads][words_per_row] and bits[n_rows][words_per_row], bit i of a row =
 * accession i (bits at or past n_acc are ignored). The leads' operands stay on the device; the rows pass in pieces (the next
 * piece's copy beside this piece's kernels), n11 on the matrix cores, one bit per pair, and the linked pairs are compacted on
 * the device into records {row, kmer = 0, lead, n1 of the row, n11, pad = 0}: rows ascending (row = the index into bits), leads
 * ascending within a row, the same bytes in every run. *n_out gets the count of all records; the first min(cap, *n_out) of them
 * are written to records_out. Checked before any device call (KGWAS_ERR_ARG): a null lead_bits or n_out, null bits with
 * n_rows > 0, null records_out with cap > 0, n_acc of 0 or above 8192, n_leads of 0 or above 4096, words_per_row below
 * ceil(n_acc / 64), r2_millionths of 0 or above 1000000. KGWAS_PROXY_PIECE_ROWS (rows per piece, at most 2^18) and
 * KGWAS_PROXY_RECORDS (records of the device buffer, default 2^20; a piece with more is drained in rounds) are the tests' hooks.
 * kgwas_proxy_kmers_run: the tool. leads_path is a list of k-mers, one per line, or a clump_kmers output (known by its header:
 * the distinct values of its column `lead`, in clump order). Refused by name (KGWAS_ERR_FORMAT) before the table is opened: a
 * k-mer of another length than kmer_len, with an illegal letter, or given twice (in a list). The leads' rows come from
 * <table_base>.table by kgwas_filter_kmers' search (a lead the table lacks is an error that names it); r2 is taken over the
 * accessions of pheno_path in its order (NULL: every accession of the table), 1 to 8192 of them; then ONE pass over the table.
 * out_path gets the header "lead kmer r2 phase n1 n11 row" (tabs) and one line per kept proxy, grouped by lead in the leads'
 * order and within a lead in table-row order: the lead as its file spells it, the proxy's k-mer, r2 (%.6f of num / den), phase
 * (+ or -: the sign of n n11 - ca cb), n1 of the proxy, n11 with the lead, the table row. Per lead the first max_per_lead
 * proxies in table order are kept, the rest only counted. out_path + ".log.txt": the inputs, one line "lead <k-mer> <kept>
 * <found>" per lead, the counters and the times. *st (may be NULL) is written when the call succeeds.
 * ---------------------------------------------------------------------------------- */
typedef struct kgwas_proxy_record {
    uint64_t row, kmer;
    uint32_t lead, n1, n11, pad;
} kgwas_proxy_record;
typedef struct kgwas_proxy_stats {
    uint64_t accessions, leads, rows_read, pairs_tested, proxies_found, proxies_kept, drain_rounds;
    double search_ms, kernel_ms, copy_ms, total_ms; /* the leads' table search, the kernels and the pieces' copies (events), all */
} kgwas_proxy_stats;
int kgwas_kmers_ld_proxies(const uint64_t* lead_bits, uint64_t n_leads, const uint64_t* bits, uint64_t n_rows, uint64_t words_per_row,
                           uint64_t n_acc, uint32_t r2_millionths, int32_t device, kgwas_proxy_record* records_out, uint64_t cap,
                           uint64_t* n_out);
int kgwas_proxy_kmers_run(const char* table_base, uint32_t kmer_len, const char* pheno_path, const char* leads_path, uint32_t r2_millionths,
                          uint64_t max_per_lead, int32_t device, const char* out_path, kgwas_proxy_stats* st);

/* ------------------------------------------------------------------------------------
 * locate_kmers: the genome positions of k-mers, exact or with one mismatch - the step after proxy_kmers: a k-mer with a p-value
 * becomes a point on a Manhattan plot once it has a contig and a position. A tool of this project's own. An associated k-mer
 * usually carries the non-reference allele and does not occur in the reference; with one mismatch allowed it lands on its locus
 * and the mismatching base is the variant.
 *
 * Definitions. The BASE STREAM is kgwas_count_kmers_bases': bytes, A C G T in either case are bases, every other byte separates.
 * A WINDOW at offset p is k consecutive base bytes; its code a has A=0, C=1, G=2, T=3, two bits per base, first base most
 * significant. QUERY i is k letters: f_i the code of the letters as spelled, r_i the code of their reverse complement. Its
 * PATTERNS are (f_i, strand 0 = +) and, unless r_i == f_i, (r_i, strand 1 = -). Two queries are the same k-mer when their
 * canonical codes (kgwas_kmer_encode) are equal. With d = mismatches in {0, 1} a HIT is a (window, pattern) pair whose codes
 * differ in h <= d base positions; its record is {pos = p, kmer = i, strand, mismatches = h, offset, pad = 0}, offset 0 for h = 0,
 * else the 1-based index, in the window as the reference spells it, of the differing base. One window can hit several queries and,
 * with d = 1, both patterns of one query: each pair is one record. Records come in ascending pos, then kmer, then strand: the same
 * bytes in every run.
 *
 * kgwas_locate_kmers_bases: the array level. bases[n_bytes] is host memory, or device memory of `device` when on_device != 0;
 * codes[n_kmers] the f_i. The patterns are sorted once and stay on the device (d = 1: by their first ceil(k / 2) and by their last
 * floor(k / 2) bases; a window looks both halves up, and a pair within one mismatch is found exactly once); the stream passes in
 * pieces that overlap by k - 1 bytes (the next piece's copy beside this piece's kernels), and the hits are compacted on the device
 * into records. *n_out gets the count of all records; the first min(cap, *n_out) are written to records_out. Checked before any
 * device call (KGWAS_ERR_ARG): null codes or n_out, null bases with n_bytes > 0, null records_out with cap > 0, kmer_len outside
 * 1..31, mismatches > 1, mismatches == 1 with kmer_len < 2, n_kmers of 0 or above 2^20, a code with bits at or above
 * 2 * kmer_len, two queries that are the same k-mer. No HIP device -> KGWAS_ERR_DEVICE. KGWAS_LOCATE_PIECE_BYTES (window positions
 * per piece, at most 2^25) and KGWAS_LOCATE_RECORDS (records of the device buffer, default 2^20; a piece with more is drained in
 * rounds) are the tests' hooks.
 * kgwas_locate_kmers_run: the tool. reference_path is FASTA in plain text: the first byte must be '>' (else KGWAS_ERR_FORMAT
 * "<path>: not FASTA"; an empty file or one without a sequence byte is KGWAS_ERR_FORMAT too); a trailing '\r' is dropped from every
 * line and a missing final newline is fine; a contig's name is its header line after '>' up to the first blank or tab (an empty
 * name or one given twice is refused by name); its sequence is the concatenation of its lines, every byte of which has a position,
 * and one separator byte goes between contigs in the stream. A file that cannot be opened -> KGWAS_ERR_IO "can't open file:
 * <path>". kmers_path is, by its first line: a tab-separated file whose header has a column `rs` (an lmm_lrt / GEMMA .assoc.txt,
 * a clump_kmers output), one whose header has a column `kmer` and no `rs` (a proxy_kmers output: its distinct values in order of
 * first appearance), or a plain list, one k-mer per line; a column `p_lrt` is carried along as text. Refused by name with the line
 * (KGWAS_ERR_FORMAT) before the reference is opened: a k-mer of another length than kmer_len, with a letter other than A, C, G, T,
 * given twice in a list or an `rs` column, a line with too few fields, no k-mer at all.
 * out_path gets the header "kmer contig pos strand mismatches offset ref alt" (tabs; a last column p_lrt when the input had one)
 * and one line per kept hit, grouped by k-mer in the input's order and within a k-mer by contig in the file's order, then
 * position, then + before -: pos is the 1-based position of the window's first base in its contig, ref the reference's letter at
 * the mismatch (upper case), alt the k-mer's base there in the reference's orientation (on strand - the complement of the query's
 * letter at k - offset, 0-based); both are '.' for an exact hit. Per k-mer the first max_per_kmer hits in that order are kept, the
 * rest only counted (0: no limit). out_path + ".log.txt": the inputs, one line "kmer <text> <kept> <found>" per query, the counters
 * and the times. No output file exists after a refusal. *st (may be NULL) is written when the call succeeds.
 * ---------------------------------------------------------------------------------- */
typedef struct kgwas_locate_record {
    uint64_t pos;
    uint32_t kmer;
    uint8_t strand, mismatches, offset, pad;
} kgwas_locate_record;
typedef struct kgwas_locate_stats {
    uint64_t contigs, bases, windows_tested, kmers, hits_found, hits_kept, kmers_without_hit, kmers_with_one_hit, drain_rounds;
    double parse_ms, copy_ms, kernel_ms, total_ms; /* the reader thread's parsing, the pieces' copies and the kernels (events), all */
} kgwas_locate_stats;
int kgwas_locate_kmers_bases(const void* bases, uint64_t n_bytes, int on_device, const uint64_t* codes, uint64_t n_kmers, uint32_t kmer_len,
                             uint32_t mismatches, int32_t device, kgwas_locate_record* records_out, uint64_t cap, uint64_t* n_out);
int kgwas_locate_kmers_run(const char* reference_path, const char* kmers_path, uint32_t kmer_len, uint32_t mismatches, uint64_t max_per_kmer,
                           int32_t device, const char* out_path, kgwas_locate_stats* st);

/* ------------------------------------------------------------------------------------
 * fetch_reads: the reads of an accession that contain listed k-mers - the other step after proxy_kmers: an associated k-mer that
 * lands nowhere in the reference (an insertion, a gene the reference lacks) is followed up by pulling the reads that hold it and
 * its proxies out of an accession's read set and assembling them locally. A tool of this project's own.
 *
 * Definitions. The BASE STREAM is bytes; A C G T in either case are bases. A READ is the bytes between one '\n' and the next: read
 * r ends at the r-th newline; reads are numbered from 0 over the whole stream, and an empty run is a read with no window. Any byte
 * other than a base or a newline ('N', '\r', ...) lies inside its read and breaks windows; it does not end the read. A WINDOW at
 * offset p of a read is k consecutive base bytes of that read; its code is locate_kmers': A=0, C=1, G=2, T=3, two bits per base,
 * first base most significant. QUERY i has the code f_i as spelled and r_i reverse-complemented; two queries with the same
 * canonical code (kgwas_kmer_encode) are the same k-mer and are refused, so a window hits at most one query. STRAND 0: the window
 * equals f_i (a palindrome counts as strand 0); strand 1: it equals r_i. Per read: n_hits is the number of its windows that hit,
 * first_pos the 0-based byte offset in the read of the first hit window, kmer and strand those of that window. A read is KEPT iff
 * n_hits >= min_hits (min_hits >= 1). Its record is {read, n_hits, first_pos, kmer, strand, pad = 0}, 24 bytes; records come in
 * ascending read, the same bytes in every run. kmer_windows[i] is the number of hit windows of query i over all reads, kept or not.
 *
 * kgwas_fetch_reads_bases: the array level. bases[n_bytes] is host memory (there is no on-device form: the pieces are cut at
 * newlines, which the host finds); codes[n_kmers] the f_i. The queries' canonical codes are sorted once and stay on the device; the
 * stream passes in pieces of at most P bytes that each end behind a newline (a last run without a newline gets one in the pinned
 * copy; the next piece's copy runs beside this piece's kernels), the hits are reduced per read on the device, and the kept reads'
 * records come back in rounds of the record buffer's size. *n_out gets the count of all records; the first min(cap, *n_out) are
 * written to records_out. kmer_windows_out[n_kmers] may be NULL. Checked before any device call (KGWAS_ERR_ARG): null codes or
 * n_out, null bases with n_bytes > 0, null records_out with cap > 0, kmer_len outside 1..31, min_hits == 0, n_kmers of 0 or above
 * 2^20, a code with bits at or above 2 * kmer_len, two queries that are the same k-mer. No HIP device -> KGWAS_ERR_DEVICE. A read
 * that does not fit a piece (its bytes and its newline) is KGWAS_ERR_ARG and names its length. KGWAS_FETCH_PIECE_BYTES (P, default
 * and at most 2^25), KGWAS_FETCH_RECORDS (records of the device buffer, default 2^20) and KGWAS_FETCH_PREFILTER (0: no presence
 * bitmap ahead of the list search; records and counts are the same either way) are the tests' hooks.
 * kgwas_fetch_reads_run: the tool. reads_path (and mates_path, may be NULL) are FASTQ or FASTA in plain text, "-" for standard
 * input, by kgwas_count_kmers_run's rules and texts: the first byte is '@' or '>' (else KGWAS_ERR_FORMAT "<path>: neither FASTA nor
 * FASTQ"); a FASTQ record is four lines with '@' and '+' at the head of its first and third line; a FASTA record's sequence is the
 * concatenation of its lines; a trailing '\r' is dropped for the stream; a missing final newline is fine; a file that cannot be
 * opened -> KGWAS_ERR_IO "can't open file: <path>". Reads enter the stream in file order. With mates, record i of the two files is
 * a pair: mate 1 is read 2 i of the stream, mate 2 read 2 i + 1; the files must have the same format, unequal record counts are
 * KGWAS_ERR_FORMAT naming the longer file, and a pair is kept iff either mate is kept. kmers_path is read as kgwas_locate_kmers_run
 * reads it (a plain list, an .assoc.txt, a clump_kmers or a proxy_kmers output), with the same refusals, before the reads are
 * opened. A UNIT is a read or, with mates, a pair; it belongs to the k-mer of its first kept read. Per k-mer the first
 * max_reads_per_kmer units in input order are written, the rest only counted (0: no limit). Outputs: out_prefix + ".fastq" or
 * ".fasta" (with mates "_1." and "_2."): the written units' records, their bytes exactly as the input has them, in input order, a
 * final newline added if the last record lacked one. out_prefix + ".reads.tsv": the header "read mate n_hits first_pos kmer strand"
 * (tabs) and one line per kept read of a written unit: the record's name up to the first blank, mate 1 or 2 (0 without mates),
 * n_hits, the 1-based first_pos, the query's text, + or -. out_prefix + ".log.txt": the inputs, one line "kmer <text> <units
 * written> <windows>" per query, the counters and the times. No output file exists after a refusal. *st (may be NULL) is written
 * when the call succeeds: reads and bases of the stream, windows_tested, kmers, windows_hit (the sum of kmer_windows), reads_kept,
 * reads_written (the kept reads of written units), pairs_written (0 without mates), kmers_without_read (queries with no unit
 * written), drain_rounds.
 * ---------------------------------------------------------------------------------- */
typedef struct kgwas_fetch_record {
    uint64_t read;
    uint32_t n_hits, first_pos, kmer;
    uint8_t strand, pad[3];
} kgwas_fetch_record;
typedef struct kgwas_fetch_stats {
    uint64_t reads, bases, windows_tested, kmers, windows_hit, reads_kept, reads_written, pairs_written, kmers_without_read, drain_rounds;
    double parse_ms, copy_ms, kernel_ms, total_ms; /* the reader thread's parsing, the pieces' copies and the kernels (events), all */
} kgwas_fetch_stats;
int kgwas_fetch_reads_bases(const void* bases, uint64_t n_bytes, const uint64_t* codes, uint64_t n_kmers, uint32_t kmer_len, uint32_t min_hits,
                            int32_t device, kgwas_fetch_record* records_out, uint64_t cap, uint64_t* n_out,
                            uint64_t* kmer_windows_out /* [n_kmers], may be NULL */);
int kgwas_fetch_reads_run(const char* reads_path, const char* mates_path /* may be NULL */, const char* kmers_path, uint32_t kmer_len,
                          uint32_t min_hits, uint64_t max_reads_per_kmer, int32_t device, const char* out_prefix, kgwas_fetch_stats* st);

/* ------------------------------------------------------------------------------------
 * Seeded synthetic table rows: kmer = row + 1, per-row frequency q/256 with
 * q in [5, 250], bits from a counter-based generator, so any shard can be produced on its GPU.
 * The host variant is the bit-identical twin used to write small .table files for the CLIs.
 * ---------------------------------------------------------------------------------- */
int kgwas_synth_rows_device(void* d_rows, uint64_t first_row, uint64_t n_rows, uint64_t n_acc_file, uint64_t seed,
                            void* hip_stream);
int kgwas_synth_rows_host(uint64_t* rows, uint64_t first_row, uint64_t n_rows, uint64_t n_acc_file, uint64_t seed);

#ifdef __cplusplus
}
#endif
#endif /* KGWAS_H */
