// env.h — every environment switch of libkgwas and its tools, in one place.
//
// OPTIONS (kgwas::opt_*): the product's run-time switches. Each one is documented in the table below, is read where it acts, and
// is walked by the test matrix (tests/, tools/fuzz_parity.py) - none selects code the default tests do not reach. Those of the
// filter plan (KGWAS_COARSE_MX .. KGWAS_NARROW, KGWAS_DEBUG_RESIDUALS) are read once per session, with the exp_* knobs the plan
// uses, by read_filter_opts (scan_plan.cpp):
//
//   KGWAS_FULL_REPLAY=1        every column is replayed push by push (no select mode)
//   KGWAS_COARSE_MX=0|1        filter family: 0 int8 (score_coarse.hip), 1 block-scaled FP4 x FP6/FP4 (score_mx.hip); unset or empty: by plan
//   KGWAS_COARSE_SLICES=1|2    force the one- / two-slice operand set (unset: chosen per chunk / by plan)
//   KGWAS_MX_S1=6              block-scaled filter: FP6 second slice instead of FP4
//   KGWAS_MXS=0..3             operand-streaming form (score_mxs.hip): never / where the resident form degenerates (default) /
//                              wherever it needs > 1 LDS group / wherever the form exists
//   KGWAS_MXS_FORM=1|2         its block shapes with one column group of up to 13 tiles
//   KGWAS_NARROW=0             1-4 columns through the wide filter instead of the narrow one
//   KGWAS_HOST_THREADS=n       replay threads of a session (overrides kgwas_scan_params.host_threads)
//   KGWAS_FINISH_THREADS=n     kgwas_scan_finish makes the select-mode columns' lists on n threads if that is more than the pool
//   KGWAS_PIN_THREADS=0|1|2    replay threads: unpinned / one CPU each / one core (SMT pair) each (default: 1 where the CPU quota covers the CPU set, else 0)
//   KGWAS_SPLIT_LAGGING=0      a column group that falls behind is not cut into single columns
//   KGWAS_FLOAT_LEAD=n         chunks a group may lag before it floats to the workers that are ahead (default 2, 0: never)
//   KGWAS_HISTORY_RING=n       record_history = 2: evictions kept per heap (default 16 sqrt(2 N))
//   KGWAS_RING_BYTES=n         size of the pinned record ring
//   KGWAS_LOG_BY_REF=0         select-mode logs copy their records instead of referring to the record ring
//   KGWAS_RECORD_COPY=memcpy|kernel   how a chunk's records reach the host ring
//   KGWAS_INGEST_PIECE_ROWS / KGWAS_INGEST_PINNED / KGWAS_INGEST_DEVICE   geometry of the streamed feed's piece rings
//   KGWAS_PIN_PLAIN=1          pinned buffers from hipHostMalloc instead of registered huge-page mappings
//   KGWAS_TRACE=1              timeline of a scan on stderr
//   KGWAS_CLI_FULL_TEARDOWN=1  the command-line tools destroy their sessions instead of _exit
//   KGWAS_AUTO_PARALLEL=1      associate_kmers: replay threads = the CPUs the process may use, whatever --parallel says
//   KGWAS_DEVICE=n             associate_snps: device ordinal
//   KGWAS_SNPKIN_CHUNK_SNPS=n  (test hook) SNPs per launch of a kgwas_snpkin session (default: about 128 MiB of per-sample values)
//   KGWAS_SNP_CHUNK_SNPS=n     (test hook) SNPs per launch of kgwas_snps_scores / kgwas_snps_best (default: up to 2^20, about 512 MiB of scores)
//   KGWAS_BED_PIECE_ROWS=n     (test hook) table rows per piece of kgwas_table_to_bed (default: up to 2^20, about 256 MiB of rows)
//   KGWAS_LMM_PIECE_ROWS=n     (test hook) table rows per piece of kgwas_lmm_test_table (default: up to 2^18, about 64 MiB of rows)
//   KGWAS_LMM_TABLE_SELECT=0   (test hook) kgwas_lmm_test_table_multi: the select kernel lets every (column, row) pair through to the host
//                              heaps (default 1: only pairs that can still enter a heap); the results are the same
//   KGWAS_LMM_PATTERN_TAG_BITS=k   (test hook) kgwas_lmm_test_table_unique: the pattern cache's tags keep only k of their 64 bits, so that
//                              they collide; the results are the same
//   KGWAS_BUILD_PIECE_ROWS=n   (test hook) all-k-mers rows per piece of kgwas_build_table (default: about 256 MiB of rows; a piece is whole key windows)
//   KGWAS_BUILD_BLOCK_WORDS=n  (test hook) words per read block of an accession's slice in kgwas_build_table (default 65 536)
//   KGWAS_LIST_PIECE_WORDS=n   (test hook) words per piece of kgwas_list_kmers (default 2^25, 256 MiB; a piece is whole key windows)
//   KGWAS_LIST_BUCKET_WORDS=n  (test hook) words aimed at per key-range bucket of a piece (default 2048); the LDS table of a bucket
//                              has twice as many slots, within 64 .. 4096
//   KGWAS_LIST_BLOCK_WORDS=n   (test hook) words per read block of a file's slice in kgwas_list_kmers (default 65 536)
//   KGWAS_COUNT_PASS_WORDS=n   (test hook) sort words per key-range pass of kgwas_count_kmers_* (default: from the bases and the free
//                              device memory, at most 2^30)
//   KGWAS_COUNT_PIECE_BYTES=n  (test hook) bytes per pinned upload piece of kgwas_count_kmers_* (default 8 MiB); when set, a file is
//                              read in blocks of 8 pieces by at most 3 threads and a device segment of the base stream holds 64 pieces
//   KGWAS_COUNT_PARSE_ONLY=1   kgwas_count_kmers_files stops behind the parse and the upload (the tool's timing mode: no output file)
//   KGWAS_LD_POPCOUNT=1        kgwas_kmers_ld / clump_kmers / proxy_kmers: the counts of common accessions come from popcount(AND) on the vector ALU
//                              instead of the matrix cores (the ablation of DESIGN.md 4.13); the results are the same
//   KGWAS_LD_TIMING=1          kgwas_kmers_ld and kgwas_kmers_ld_proxies print their kernels' time (events around them alone) on stderr
//   KGWAS_PROXY_PIECE_ROWS=n   (test hook) rows per piece of kgwas_kmers_ld_proxies / proxy_kmers (default: up to 2^18, about 64 MiB of rows)
//   KGWAS_PROXY_RECORDS=n      (test hook) records of their device record buffer (default 2^20); a piece with more is drained in rounds
//   KGWAS_FETCH_PIECE_BYTES=n  (test hook) bytes per piece of kgwas_fetch_reads_* (default and at most 2^25); a piece is whole reads
//   KGWAS_FETCH_RECORDS=n      (test hook) records of their device record buffer (default 2^20); a piece with more is drained in rounds
//   KGWAS_FETCH_PREFILTER=0|1  (test hook) without / with the presence bitmap ahead of the list search; the results are the same
//   KGWAS_FETCH_TIMING=1       kgwas_fetch_reads_bases prints its kernels' and copies' time (events) on stderr
//   KGWAS_DEBUG_SLOW_WORKER=w:pct:min_us   (test hook) slows one replay worker down
//   KGWAS_DEBUG_RESIDUALS=1    (test hook) sessions keep their filters' quantisation residuals (kgwas_scan_debug_residuals)
//   KGWAS_DEBUG_SURVIVORS=1    (test hook) filter sessions log every filtered chunk's thresholds and survivors, synchronously
//                              (kgwas_scan_debug_survivors)
//
// EXPERIMENTS (kgwas::exp_*): tuning and ablation knobs of tools/ (chunk-size policies, block sizes, prefetch distances, older
// forms of a step kept for A/B runs). They exist only in a build with -DKGWAS_EXPERIMENTS (`make EXPERIMENTS=1`); in the
// shipped library every exp_* call is its default - a compile-time constant, no getenv, and the branch it guarded folds away.
#pragma once
#include <stdlib.h>

namespace kgwas {

inline const char* opt_str(const char* name) { return getenv(name); }
inline bool opt_set(const char* name) { return opt_str(name) != nullptr; }
inline long long opt_int(const char* name, long long dflt) {
    const char* e = opt_str(name);
    return e && *e ? atoll(e) : dflt;
}

#ifdef KGWAS_EXPERIMENTS
inline const char* exp_str(const char* name) { return opt_str(name); }
inline bool exp_set(const char* name) { return opt_set(name); }
inline long long exp_int(const char* name, long long dflt) { return opt_int(name, dflt); }
inline double exp_num(const char* name, double dflt) {
    const char* e = opt_str(name);
    return e && *e ? atof(e) : dflt;
}
#else
constexpr const char* exp_str(const char*) { return nullptr; }
constexpr bool exp_set(const char*) { return false; }
constexpr long long exp_int(const char*, long long dflt) { return dflt; }
constexpr double exp_num(const char*, double dflt) { return dflt; }
#endif

}  // namespace kgwas
